"""
CPU oracle of the dominant-edge contraction (include/exaspim_affinity.h), written straight from
the rules with Python integers:

    valid_rows(edges, counts, k)    -> the indices of the rows that rule 5 does not skip
    dominant_edges_literal(edges, counts, sums, sizes, threshold)
                                    -> the indices of the contracted rows (rules 1-3 word for word), ascending
    dominant_edges(edges, counts, sums, sizes, threshold)
                                    -> the same in one pass over the rows, for large graphs
    one_round(edges, counts, sums, sizes, threshold)
                                    -> (edges' (E', 2) int32 sorted by (lo, hi), counts' int64, sums' uint64,
                                        sizes' int64 (K' + 1), map int32 (K + 1))
    is_last(k, k_new)               -> the stopping rule: the round removed fewer than max(1, K // 64)
    rounds(edges, counts, sums, sizes, threshold, limit=64)
                                    -> (the reduced graph, the composed map, [K' after each round])
    tie_heavy_graph(seed, k, n_edges)
                                    -> counts 1 .. 3, sums on a handful of values: ties everywhere
"""

import numpy as np

from premerge_ref import ONE, merge_bound


def valid_rows(edges, counts, k):
    return [e for e, ((lo, hi), c) in enumerate(zip(np.asarray(edges).reshape(-1, 2).tolist(), counts))
            if 1 <= lo <= k and 1 <= hi <= k and lo != hi and int(c) != 0]


def _mergeable_rows(edges, counts, sums, k, threshold):
    m, merge_all = merge_bound(threshold)
    rows = [(e, int(edges[e][0]), int(edges[e][1]), int(counts[e]), int(sums[e])) for e in valid_rows(edges, counts, k)]
    return [r for r in rows if merge_all or r[4] > m * r[3]]          # rule 1


def dominant_edges_literal(edges, counts, sums, sizes, threshold):
    """Rules 1-3 word for word: quadratic in the degree, for small graphs."""
    k = len(sizes) - 1
    rows = _mergeable_rows(edges, counts, sums, k, threshold)
    at = [[] for _ in range(k + 1)]
    for r in rows:
        at[r[1]].append(r)
        at[r[2]].append(r)

    def dominates(r, f):                                              # rule 2: strict, in integers
        return all(r[4] * o[3] > o[4] * r[3] for o in at[f] if o[0] != r[0])

    return [r[0] for r in rows if dominates(r, r[1]) and dominates(r, r[2])]      # rule 3


def dominant_edges(edges, counts, sums, sizes, threshold):
    """The same in one pass: e dominates at f iff it is the only mergeable row at f with the largest mean."""
    k = len(sizes) - 1
    rows = _mergeable_rows(edges, counts, sums, k, threshold)
    top = [None] * (k + 1)                         # [count, sum, row, rows of that mean]
    for r in rows:
        for f in r[1:3]:
            t = top[f]
            if t is None or r[4] * t[0] > t[1] * r[3]:
                top[f] = [r[3], r[4], r[0], 1]
            elif r[4] * t[0] == t[1] * r[3]:
                t[3] += 1
    chosen = [r[0] for r in rows if all(top[f][2] == r[0] and top[f][3] == 1 for f in r[1:3])]
    ends = [int(f) for e in chosen for f in edges[e]]
    assert len(ends) == len(set(ends)), "the contracted edges are no matching"
    return chosen


def one_round(edges, counts, sums, sizes, threshold):
    edges = np.asarray(edges).reshape(-1, 2)
    k = len(sizes) - 1
    head = list(range(k + 1))
    for e in dominant_edges(edges, counts, sums, sizes, threshold):
        lo, hi = sorted(int(v) for v in edges[e])
        head[hi] = lo
    number, mapping = {}, np.zeros(k + 1, np.int32)
    for f in range(1, k + 1):                      # ascending: a set is numbered when its smallest member comes
        if head[f] not in number:
            number[head[f]] = len(number) + 1
        mapping[f] = number[head[f]]
    new_sizes = [0] * (len(number) + 1)
    new_sizes[0] = int(sizes[0])
    for f in range(1, k + 1):
        new_sizes[mapping[f]] += int(sizes[f])
    pooled = {}
    for e in valid_rows(edges, counts, k):
        a, b = int(mapping[int(edges[e][0])]), int(mapping[int(edges[e][1])])
        if a == b:
            continue
        key = (min(a, b), max(a, b))
        old = pooled.get(key, (0, 0))
        pooled[key] = (old[0] + int(counts[e]), old[1] + int(sums[e]))
    keys = sorted(pooled)
    return (np.array(keys, np.int32).reshape(-1, 2), np.array([pooled[q][0] for q in keys], np.int64),
            np.array([pooled[q][1] for q in keys], np.uint64), np.array(new_sizes, np.int64), mapping)


def is_last(k, k_new):
    return k - k_new < max(1, k // 64)


def rounds(edges, counts, sums, sizes, threshold, limit=64):
    graph = (np.asarray(edges, np.int32).reshape(-1, 2), np.asarray(counts, np.int64), np.asarray(sums, np.uint64),
             np.asarray(sizes, np.int64))
    composed = np.arange(len(sizes), dtype=np.int32)
    history = []
    for _ in range(limit):
        k = len(graph[3]) - 1
        *graph, mapping = one_round(*graph, threshold)
        graph = tuple(graph)
        composed = mapping[composed]
        history.append(len(graph[3]) - 1)
        if is_last(k, history[-1]):
            break
    return graph, composed, history


def tie_heavy_graph(seed, k, n_edges, max_size=40):
    """
    A random region graph of k fragments, about n_edges distinct pairs, counts 1 .. 3 and sums j * ONE / 4
    with j in 0 .. 4 * count: the means are the multiples of 1/4, 1/8 and 1/12 in 0 .. 1, which meet across
    counts, so most maxima tie. Sizes 1 .. max_size.
    """
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, max_size + 1, k + 1).astype(np.int64)
    if k < 2:
        return np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint64), sizes
    a = rng.integers(1, k + 1, n_edges)
    b = rng.integers(1, k + 1, n_edges)
    keep = a != b
    keys = np.unique((np.minimum(a, b)[keep].astype(np.int64) << 32) | np.maximum(a, b)[keep])
    edges = np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    counts = rng.integers(1, 4, len(edges)).astype(np.int64)
    sums = (rng.integers(0, 4 * counts + 1) * (ONE // 4)).astype(np.uint64)
    return edges, counts, sums, sizes
