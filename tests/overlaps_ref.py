"""
Oracles of the overlap table of two label volumes, written from the definition, and the scores of
overlap_scores written a second time, independently of the package. No GPU and no import of the package.

The definition: v' = v if v > 0 else 0; for every voxel count[(a', b')] += 1; the pair is ordered.
    table_unique(a, b)     (A) numpy.unique on the keys a' * 2^32 + b' packed into int64
    table_dict(a, b)       (B) a plain Python loop into a dict
both give (pairs int32 (P, 2) sorted by (a', b'), counts int64 (P,)).
    scores(pairs, counts, background)   per-row loops, math.log2 and fractions.Fraction: the Rand quantities as
                                        Fractions, the entropies as floats summed row by row
    old_agreement(a, b)    tools/watershed_rate.py's former agreement() rule restated in numpy
    volumes(seed)          the seeded pairs of volumes the CPU tests run on
"""

import math
from fractions import Fraction

import numpy as np

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def fold(v):
    v = np.asarray(v)
    assert v.dtype == np.int32
    return np.where(v > 0, v, 0).astype(np.int64)


def table_unique(a, b):
    a, b = fold(a).ravel(), fold(b).ravel()
    assert a.shape == b.shape
    keys, counts = np.unique(a << 32 | b, return_counts=True)      # both halves < 2^31: no sign trouble, sorted
    pairs = np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, counts.astype(np.int64)


def table_dict(a, b):
    table = {}
    for x, y in zip(np.asarray(a).ravel().tolist(), np.asarray(b).ravel().tolist()):
        key = (x if x > 0 else 0, y if y > 0 else 0)
        table[key] = table.get(key, 0) + 1
    keys = sorted(table)
    return (np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([table[k] for k in keys], dtype=np.int64))


def kept_rows(pairs, counts, background):
    rows = [(int(i), int(j), int(c)) for (i, j), c in zip(np.asarray(pairs).tolist(), np.asarray(counts).tolist())]
    if background == "a":
        return [r for r in rows if r[0] != 0]
    if background == "both_zero":
        return [r for r in rows if (r[0], r[1]) != (0, 0)]
    assert background == "none"
    return rows


def scores(pairs, counts, background):
    """The fields of overlap_scores; the Rand quantities as Fractions (None where the issue's rule for a zero
    denominator applies: the caller checks those against 1.0 / 0.0)."""
    everything = kept_rows(pairs, counts, "none")
    rows = kept_rows(pairs, counts, background)
    n = 0
    for _, _, c in rows:
        n += c
    a_sizes, b_sizes = {}, {}
    for i, j, c in rows:
        a_sizes[i] = a_sizes.get(i, 0) + c
        b_sizes[j] = b_sizes.get(j, 0) + c
    # entropies in bits, from probabilities: H(A,B), H(A), H(B)
    h_ab = -sum(c / n * math.log2(c / n) for _, _, c in rows) if n else 0.0
    h_a = -sum(c / n * math.log2(c / n) for c in a_sizes.values()) if n else 0.0
    h_b = -sum(c / n * math.log2(c / n) for c in b_sizes.values()) if n else 0.0
    s_ij = sum(c**2 for _, _, c in rows)
    s_a = sum(c**2 for c in a_sizes.values())
    s_b = sum(c**2 for c in b_sizes.values())
    precision = Fraction(s_ij - n, s_b - n) if s_b - n else None
    recall = Fraction(s_ij - n, s_a - n) if s_a - n else None
    p, r = (Fraction(1) if v is None else v for v in (precision, recall))
    error = 1 - 2 * p * r / (p + r) if p + r else None
    # pairs of voxels together in both, together in neither, over all pairs
    both = Fraction(s_ij - n, 2)
    only_a, only_b = Fraction(s_a - n, 2) - both, Fraction(s_b - n, 2) - both
    all_pairs = Fraction(n * (n - 1), 2)
    rand = (all_pairs - only_a - only_b) / all_pairs if all_pairs else None
    total = sum(c for _, _, c in everything)
    zero = sum(c for i, j, c in everything if i == 0 and j == 0)
    largest = 0
    for i in sorted({r[0] for r in everything if r[0] >= 1}):
        largest += max(c for ii, _, c in everything if ii == i)
    per_a, per_b = {}, {}
    for i, j, _ in rows:
        per_a[i] = per_a.get(i, 0) + 1
        per_b[j] = per_b.get(j, 0) + 1
    return {
        "n": n, "segments_a": len(a_sizes), "segments_b": len(b_sizes), "pairs": len(rows),
        "voi_split": h_ab - h_a, "voi_merge": h_ab - h_b, "voi": 2 * h_ab - h_a - h_b,
        "rand_precision": precision, "rand_recall": recall, "adapted_rand_error": error, "rand_index": rand,
        "largest_overlap_agreement": Fraction(largest, total - zero) if total - zero else None,
        "same_partition": set(per_a.values()) <= {1} and set(per_b.values()) <= {1},
    }


def old_agreement(exact, merged):
    """Over the voxels that are foreground in either: the sum over the segments >= 1 of "exact" of the largest
    overlap with one value of "merged", divided by the voxel count. The packed-unique rule of the tool."""
    exact, merged = np.asarray(exact).ravel(), np.asarray(merged).ravel()
    either = (exact > 0) | (merged > 0)
    total = int(either.sum())
    if total == 0:
        return 1.0
    a, b = exact[either].astype(np.int64), merged[either].astype(np.int64)
    a, b = np.maximum(a, 0), np.maximum(b, 0)
    base = int(b.max()) + 1
    keys, counts = np.unique(a * base + b, return_counts=True)
    seg = keys // base
    best = np.zeros(int(seg.max()) + 1, dtype=np.int64)
    np.maximum.at(best, seg, counts)
    return float(best[1:].sum()) / total


def blocky(rng, shape, top, run):
    """Labels 0 .. top that are constant along x in runs of random length up to "run"."""
    n = int(np.prod(shape))
    cuts = np.cumsum(rng.integers(1, run + 1, size=n))
    cuts = cuts[cuts < n]
    ids = rng.integers(0, top + 1, size=len(cuts) + 1)
    return np.repeat(ids, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.int32).reshape(shape)


def volumes(seed):
    """(a, b) int32 of one small seeded shape: runs of labels, with negatives, INT32_MIN, 2^31 - 1 and sparse
    ids mixed in according to the seed."""
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(1, (6, 9, 40)))
    a = blocky(rng, shape, 1 + seed % 7, 1 + seed % 11)
    b = blocky(rng, shape, 1 + seed % 5, 1 + seed % 13)
    if seed % 2:      # b follows a with a few voxels moved: close to the same partition
        b = np.where(rng.random(shape) < 0.9, a, b).astype(np.int32)
    if seed % 3 == 0:      # sparse ids: 2048 apart, and the two ends of the range
        a = np.where(a > 0, 2048 * (a - 1) + 1, a).astype(np.int32)
        b = np.where(b == 1, INT32_MAX, b).astype(np.int32)
    if seed % 4 == 0:      # what folds to 0
        a = np.where(rng.random(shape) < 0.1, -rng.integers(1, 50, size=shape), a).astype(np.int32)
        b = np.where(rng.random(shape) < 0.05, INT32_MIN, b).astype(np.int32)
    if seed % 5 == 0:
        a = np.where(rng.random(shape) < 0.05, INT32_MAX, a).astype(np.int32)
    return a, b
