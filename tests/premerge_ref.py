"""
CPU oracle of the size-floor pre-merge (include/exaspim_affinity.h), written straight from the
definition with Python integers:

    merge_bound(threshold)          -> (m, merge_all), as exaspim_agglomerate computes them
    choices(edges, counts, sums, sizes, threshold, floor)
                                    -> choice[0 .. K] after rules 1-4 (choice[f] = f: none)
    roots(choice)                   -> root[0 .. K] by following choices; raises on a cycle
    one_round(edges, counts, sums, sizes, threshold, floor)
                                    -> (edges' (E', 2) int32 sorted by (lo, hi), counts' int64, sums' uint64,
                                        sizes' int64 (K' + 1), map int32 (K + 1), depth of the longest chain)
    rounds(edges, counts, sums, sizes, threshold, floor, limit=4)
                                    -> (the reduced graph, the composed map, [K' after each round])
    random_graph(seed, k, n_edges, levels)
                                    -> a tie-heavy random graph for the tests
"""

import numpy as np

ONE = 1 << 24


def merge_bound(threshold):
    md = float(np.rint((1.0 - float(np.float32(threshold))) * ONE))
    return (0 if md < 0 else min(int(md), ONE)), md < 0


def choices(edges, counts, sums, sizes, threshold, floor):
    k = len(sizes) - 1
    m, merge_all = merge_bound(threshold)
    best = [None] * (k + 1)                        # (count, sum, neighbour)
    for (lo, hi), c, s in zip(edges, counts, sums):
        lo, hi, c, s = int(lo), int(hi), int(c), int(s)
        if not (merge_all or s > m * c):
            continue
        for f, g in ((lo, hi), (hi, lo)):
            if not int(sizes[f]) < floor:
                continue
            b = best[f]
            if b is None or s * b[0] > b[1] * c or (s * b[0] == b[1] * c and g < b[2]):
                best[f] = (c, s, g)
    choice = [f if best[f] is None else best[f][2] for f in range(k + 1)]
    mutual = [f for f in range(1, k + 1) if choice[f] != f and choice[choice[f]] == f and f < choice[f]]
    for f in mutual:
        choice[f] = f
    return choice


def roots(choice):
    """root[f] and the length of the longest chain; a cycle is an AssertionError."""
    n = len(choice)
    root, depth = [None] * n, [0] * n
    for f in range(n):
        path, g = [], f
        while root[g] is None and choice[g] != g:
            path.append(g)
            g = choice[g]
            assert len(path) <= n, "the choices hold a cycle"
        if root[g] is None:
            root[g] = g
        base, d = root[g], depth[g]
        for h in reversed(path):
            d += 1
            root[h], depth[h] = base, d
    return root, max(depth)


def one_round(edges, counts, sums, sizes, threshold, floor):
    k = len(sizes) - 1
    root, depth = roots(choices(edges, counts, sums, sizes, threshold, floor))
    number, mapping = {}, np.zeros(k + 1, np.int32)
    for f in range(1, k + 1):                      # ascending: a set is numbered when its smallest member comes
        if root[f] not in number:
            number[root[f]] = len(number) + 1
        mapping[f] = number[root[f]]
    new_sizes = [0] * (len(number) + 1)
    new_sizes[0] = int(sizes[0])
    for f in range(1, k + 1):
        new_sizes[mapping[f]] += int(sizes[f])
    pooled = {}
    for (lo, hi), c, s in zip(edges, counts, sums):
        a, b = int(mapping[int(lo)]), int(mapping[int(hi)])
        if a == b:
            continue
        key = (min(a, b), max(a, b))
        old = pooled.get(key, (0, 0))
        pooled[key] = (old[0] + int(c), old[1] + int(s))
    keys = sorted(pooled)
    return (np.array(keys, np.int32).reshape(-1, 2), np.array([pooled[q][0] for q in keys], np.int64),
            np.array([pooled[q][1] for q in keys], np.uint64), np.array(new_sizes, np.int64), mapping, depth)


def random_graph(seed, k, n_edges, levels, max_size=40):
    """
    A random region graph of k fragments whose affinities take only "levels" values, so that most maxima
    tie: about n_edges distinct pairs, counts 1 .. 6, every voxel edge's q one of the levels, sizes 1 .. max_size.
    """
    rng = np.random.default_rng(seed)
    if k < 2:
        return (np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint64),
                rng.integers(1, max_size + 1, k + 1).astype(np.int64))
    a = rng.integers(1, k + 1, n_edges)
    b = rng.integers(1, k + 1, n_edges)
    keep = a != b
    keys = np.unique((np.minimum(a, b)[keep].astype(np.int64) << 32) | np.maximum(a, b)[keep])
    edges = np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    counts = rng.integers(1, 7, len(edges)).astype(np.int64)
    step = ONE // (levels - 1)
    sums = np.array([int(rng.integers(0, levels, c).sum()) * step for c in counts], np.uint64)
    return edges, counts, sums, rng.integers(1, max_size + 1, k + 1).astype(np.int64)


def rounds(edges, counts, sums, sizes, threshold, floor, limit=4):
    graph = (np.asarray(edges, np.int32).reshape(-1, 2), np.asarray(counts, np.int64), np.asarray(sums, np.uint64),
             np.asarray(sizes, np.int64))
    composed = np.arange(len(sizes), dtype=np.int32)
    history = []
    for _ in range(limit):
        k = len(graph[3]) - 1
        *graph, mapping, _ = one_round(*graph, threshold, floor)
        graph = tuple(graph)
        composed = mapping[composed]
        history.append(len(graph[3]) - 1)
        if history[-1] == k:
            break
    return graph, composed, history
