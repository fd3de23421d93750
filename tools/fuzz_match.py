"""Randomised parity of the features matcher (isx_match_features) against its NumPy model (tests/helpers/match_np.py): matches, counts,
points and knn with np.array_equal.

    python tools/fuzz_match.py --seconds 600 --seed 20261119 [--out profiles/fuzz_match_600s.json]

The generator (no GPU needed: tests/test_match_model.py checks it).  case(seed) draws one of CLASSES:
    tiny          4 .. 12 rows an image
    tile_edges    rows at a multiple of QUERY_BLOCK / TRAIN_TILE, one less, one more
    chunk_edges   rows at a multiple of TRAIN_CHUNK, one less, one more
    duplicates    filler rows repeated (ties of the first and of the second neighbour)
    clustered     filler rows a few bits from one base row (small distances, many ties, ratio tests either side of the bound)
    many          3 .. 5 images, a mask, an image without rows now and then
    split         one image of 8192 k - 1, 8192 k or 8192 k + 1 rows, k = 1 .. 3, against one of 4 .. 300, in either order (past 32 chunks of
                  TRAIN_CHUNK the chunk of a work item grows: 512 and 768 rows, last chunks that are not whole tiles, up to 32 partials
                  a query), with `duplicates` or `clustered` filler now and then
case(seed) without a class draws one of the first six, as it did before `split`; a soak takes all seven in turn (scheduled()).
Every pair of every case carries planted structure among fresh random rows (which lie about 128 +- 8 bits from every other row, so what
is planted stays isolated): mutual matches at distances 0, 1, .. (at most 16) - accepted both ways -, a fork (two rows of `to` 3 disjoint
flips from one row of `from`: 1->2 ties and is rejected, both 2->1 matches are appended) and a reverse fork (two rows of `from` 4 flips
from one row of `to`: two 1->2 matches to one train row, 2->1 rejected).  match_conf is drawn from {0, 0.3, 0.5, 0.65} and [0, 0.9]: the
planted distances pass the ratio test against a second neighbour 60 bits away throughout.  Layouts: host or device mats, dense or with an odd
pointer and a step of 33 / 40 bytes, outputs dense or padded."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from helpers import match_np as M  # noqa: E402
from imagestitch_amd.matcher import QUERY_BLOCK, TRAIN_CHUNK, TRAIN_TILE  # noqa: E402

BASE_CLASSES = ("tiny", "tile_edges", "chunk_edges", "duplicates", "clustered", "many")
CLASSES = BASE_CLASSES + ("split",)
SPLIT_ROWS = TRAIN_CHUNK * 32      # 8192: the rows of a train image from which on the chunk of a work item grows
CONFS = (0.0, 0.3, 0.5, 0.65)
ROWS_PER_PAIR = 4          # rows of an image the planted structure of one pair needs at least
MAX_MUTUAL = 17            # distances 0 .. 16


def flip(row, bits):
    """row (32 uint8) with the named bit positions XORed."""
    out = np.array(row, np.uint8)
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def plant(rng, descs, free, i, j, left):
    """Plants one pair's structure into rows of images i and j taken from their free lists (left[i]: the pairs of image i still to be
    planted, this one included - each gets an even share of the free rows); returns what was planted."""
    fi, fj = free[i], free[j]
    m = int(min(MAX_MUTUAL, len(fi) // left[i] - 3, len(fj) // left[j] - 3))
    left[i] -= 1
    left[j] -= 1
    assert m >= 1, "an image needs %d free rows a pair" % ROWS_PER_PAIR
    a, b = descs[i], descs[j]
    planted = dict(mutual=[], fork=None, reverse_fork=None)
    for t in range(m):
        ra, rb = fi.pop(), fj.pop()
        a[ra] = random_rows(rng, 1)[0]
        b[rb] = flip(a[ra], rng.permutation(256)[:t])
        planted["mutual"].append((ra, rb, t))
    ra, rb1, rb2 = fi.pop(), fj.pop(), fj.pop()
    a[ra] = random_rows(rng, 1)[0]
    bits = rng.permutation(256)[:6]
    b[rb1], b[rb2] = flip(a[ra], bits[:3]), flip(a[ra], bits[3:])
    planted["fork"] = (ra, rb1, rb2)
    rb, ra1, ra2 = fj.pop(), fi.pop(), fi.pop()
    b[rb] = random_rows(rng, 1)[0]
    bits = rng.permutation(256)[:8]
    a[ra1], a[ra2] = flip(b[rb], bits[:4]), flip(b[rb], bits[4:])
    planted["reverse_fork"] = (rb, ra1, ra2)
    return planted


def build(rng, rows, pairs, filler="random"):
    """Descriptor arrays of the given row counts with every pair's planted structure and `filler` rows elsewhere."""
    descs = [np.zeros((n, 32), np.uint8) for n in rows]
    free = [list(rng.permutation(n)) for n in rows]
    left = [sum(1 for p in pairs if k in p) for k in range(len(rows))]
    planted = [plant(rng, descs, free, i, j, left) for i, j in pairs]
    for d, f in zip(descs, free):
        f = list(f)
        if not f:
            continue
        if filler == "clustered":
            base = random_rows(rng, 1)[0]
            for r in f:
                d[r] = flip(base, rng.permutation(256)[:int(rng.integers(0, 7))])
        else:
            d[f] = random_rows(rng, len(f))
            if filler == "duplicates" and len(f) >= 2:
                fa = np.asarray(f)                         # (the same draws as from the list, without converting it every time)
                for _ in range(max(1, len(f) // 3)):
                    src, dst = rng.choice(fa, 2, replace=False)
                    d[dst] = d[src]
    return descs, planted


def _edge(rng, unit, most=3):
    return max(ROWS_PER_PAIR, int(unit * rng.integers(1, most + 1) + rng.integers(-1, 2)))


def case(seed, cls=None):
    """One case: dict(cls, descriptors, keypoints, img_sizes, pairs, mask, match_conf, planted)."""
    rng = np.random.default_rng(seed)
    cls = cls or BASE_CLASSES[int(rng.integers(len(BASE_CLASSES)))]
    mask = None
    filler = cls if cls in ("duplicates", "clustered") else "random"
    if cls == "tiny":
        rows = [int(rng.integers(4, 13)) for _ in range(2)]
    elif cls == "tile_edges":
        rows = [_edge(rng, QUERY_BLOCK), _edge(rng, TRAIN_TILE)]
    elif cls == "chunk_edges":
        rows = [_edge(rng, TRAIN_CHUNK, 2), _edge(rng, TRAIN_CHUNK, 2)]
    elif cls in ("duplicates", "clustered"):
        rows = [int(rng.integers(8, 300)) for _ in range(2)]
    elif cls == "split":
        rows = [SPLIT_ROWS * int(rng.integers(1, 4)) + int(rng.integers(-1, 2)), int(rng.integers(4, 301))]
        if rng.random() < 0.5:
            rows.reverse()
        filler = ("random", "random", "duplicates", "clustered")[int(rng.integers(4))]
    else:
        n = int(rng.integers(3, 6))
        rows = [int(rng.integers(ROWS_PER_PAIR * (n - 1), 200)) for _ in range(n)]
        if rng.random() < 0.4:
            rows[int(rng.integers(n))] = 0
        mask = (rng.random((n, n)) < 0.75).astype(np.uint8)
        if not any(mask[i, j] for i, j in M.near_pairs(rows)):
            mask = None
    pairs = M.near_pairs(rows, mask)
    descs, planted = build(rng, rows, pairs, filler)
    sizes = [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000))) for _ in rows]
    kps = [(rng.random((n, 2)) * np.array(s)).astype(np.float32) for n, s in zip(rows, sizes)]
    conf = float(CONFS[int(rng.integers(len(CONFS)))]) if rng.random() < 0.7 else float(np.float32(rng.random() * 0.9))
    return dict(cls=cls, descriptors=descs, keypoints=kps, img_sizes=sizes, pairs=pairs, mask=mask, match_conf=conf, planted=planted,
                layout_seed=int(rng.integers(1 << 30)))


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
def _place(rng, a, device, strided):
    """`a` (2-D) as a host array or a device tensor, dense or - strided - as a view with an odd first byte (1-byte elements) and padded rows.
    Returns (the mat to pass, a function that gives its content back as a NumPy array)."""
    import torch
    a = np.ascontiguousarray(a)
    h, w = a.shape
    es = a.dtype.itemsize
    if strided:
        pad = int(rng.choice([1, 8])) if es == 1 else 4 * int(rng.integers(1, 4))
        lead = 1 if es == 1 else 4
        raw = np.full(lead + max(h, 1) * (w * es + pad) + 8, 0xA5, np.uint8)
        view = np.ndarray((h, w), a.dtype, buffer=raw, offset=lead, strides=(w * es + pad, es))
        view[...] = a
        if device:
            traw = torch.from_numpy(raw).cuda()
            tv = traw[lead:lead + (max(h, 1) - 1) * (w * es + pad) + w * es].view(getattr(torch, a.dtype.name))
            tv = tv.as_strided((h, w), ((w * es + pad) // es, 1)) if es > 1 else traw.as_strided((h, w), (w + pad, 1), lead)
            return tv, lambda: tv.cpu().numpy()
        return view, lambda: view.copy()
    if device:
        t = torch.from_numpy(a.copy()).cuda()
        return t, lambda: t.cpu().numpy()
    c = a.copy()
    return c, lambda: c.copy()


SENTINEL = -7777


def run_case(c, rng=None):
    """Runs one case through the library in a random layout and compares with the model.  Returns a list of differences (empty: equal)."""
    import torch
    from imagestitch_amd import matcher
    rng = rng or np.random.default_rng(c["layout_seed"])
    pairs, descs = c["pairs"], c["descriptors"]
    if not pairs:
        return []
    want = M.match_model(descs, pairs, c["match_conf"], c["keypoints"], c["img_sizes"])
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
    matcher.match_features(d_in, pairs, c["match_conf"], [m[0] for m in ms], cnt[0], k_in, c["img_sizes"] if with_points else None,
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


def scheduled(seed, n):
    """(case seed, class) of a soak's n-th case: the classes in turn."""
    return int(seed) * 1000003 + n, CLASSES[n % len(CLASSES)]


def run(seconds, seed, verbose=False, progress_path=None):
    """Draws cases (the classes in turn) for `seconds` and compares the library with the model.  Returns a summary dict; progress_path: a file
    that gets the running counts every 30 seconds."""
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
        s, cls = scheduled(seed, n)
        c = case(s, cls)
        bad = run_case(c)
        per[cls] += 1
        pairs += len(c["pairs"])
        n += 1
        if bad:
            failing.append(dict(seed=s, cls=cls, differences=bad[:4]))
            if verbose:
                print("MISMATCH", s, cls, bad[:4], flush=True)
    return dict(tool="fuzz_match", seconds=round(time.time() - t0, 1), seed=int(seed), cases=n, pairs=pairs, mismatches=len(failing), per_class=per,
                failing_seeds=failing[:20], device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--seed", type=int, default=20261119)
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
