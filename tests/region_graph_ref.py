"""
CPU oracles of the mean-affinity agglomeration (include/exaspim_affinity.h), written the
plain way:

    quantise(a)                     q(a) = rint(clamp(float32(a), 0, 1) * 2^24), NaN -> 0, as uint64
    region_graph(labels, aff, n_labels=None)
                                    -> (edges (E, 2) int32 sorted by (lo, hi), counts int64, sums uint64,
                                        sizes int64 (n_labels + 1)): np.unique on 64-bit keys, np.add.at
    agglomerate(edges, counts, sums, sizes, threshold, min_size)
                                    -> (table int32 (K + 1), S): scans all current edges for the best one
                                       each step, Python integers for every comparison
    agglomerate_affinities(aff, thresholds, min_size, fragment_threshold)
                                    -> labels int32, composed from these and components_ref.components
"""

import numpy as np

import components_ref

ONE = 1 << 24


def quantise(a):
    a = np.asarray(a).astype(np.float32)
    a = np.where(np.isnan(a), np.float32(0), a)
    a = np.clip(a, np.float32(0), np.float32(1))
    return np.rint(a * np.float32(ONE)).astype(np.uint64)


def region_graph(labels, aff, n_labels=None):
    labels = np.asarray(labels)
    aff = np.asarray(aff)
    assert labels.ndim == 3 and aff.shape == (3,) + labels.shape
    if n_labels is None:
        n_labels = max(int(labels.max(initial=0)), 0)
    lab = labels.astype(np.int64)
    valid = (lab >= 0) & (lab <= n_labels)
    sizes = np.bincount(lab[valid], minlength=n_labels + 1).astype(np.int64)
    keys, qs = [], []
    for c in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[c], hi[c] = slice(0, -1), slice(1, None)
        la, lb = lab[tuple(lo)], lab[tuple(hi)]
        m = (la > 0) & (lb > 0) & (la != lb) & (la <= n_labels) & (lb <= n_labels)
        keys.append((np.minimum(la, lb)[m] << 32) | np.maximum(la, lb)[m])
        qs.append(quantise(aff[c][tuple(lo)][m]))
    keys, qs = np.concatenate(keys), np.concatenate(qs)
    uniq, inverse = np.unique(keys, return_inverse=True)
    counts = np.zeros(uniq.size, np.int64)
    sums = np.zeros(uniq.size, np.uint64)
    np.add.at(counts, inverse, 1)
    np.add.at(sums, inverse, qs)
    edges = np.stack([uniq >> 32, uniq & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    return edges, counts, sums, sizes


def agglomerate(edges, counts, sums, sizes, threshold, min_size):
    k = len(sizes) - 1
    m = int(np.rint((1.0 - float(np.float32(threshold))) * ONE))
    cur = {(int(lo), int(hi)): [int(c), int(s)] for (lo, hi), c, s in zip(edges, counts, sums)}
    root = list(range(k + 1))
    while cur:
        best = None
        for (lo, hi), (c, s) in cur.items():
            if best is None:
                best = (lo, hi, c, s)
                continue
            left, right = s * best[2], best[3] * c          # s / c against best's mean
            if left > right or (left == right and (lo, hi) < (best[0], best[1])):
                best = (lo, hi, c, s)
        u, v, c, s = best
        if not s > m * c:
            break
        del cur[(u, v)]
        pooled = {}
        for (lo, hi), cs in cur.items():
            lo, hi = (u if lo == v else lo), (u if hi == v else hi)
            key = (min(lo, hi), max(lo, hi))
            if key in pooled:
                pooled[key] = [pooled[key][0] + cs[0], pooled[key][1] + cs[1]]
            else:
                pooled[key] = cs
        cur = pooled
        root = [u if r == v else r for r in root]
    total = [0] * (k + 1)
    for label in range(1, k + 1):
        total[root[label]] += int(sizes[label])
    table = np.zeros(k + 1, np.int32)
    count = 0
    for label in range(1, k + 1):      # a root is its set's smallest id, so it comes first
        if root[label] == label:
            if total[label] > min_size:
                count += 1
                table[label] = count
        else:
            table[label] = table[root[label]]
    return table, count


def agglomerate_affinities(aff, agglomeration_thresholds=(0.6, 0.8, 0.9), min_segment_size=100,
                           fragment_threshold=0.5):
    thresholds = list(agglomeration_thresholds)
    assert all(b >= a for a, b in zip(thresholds, thresholds[1:]))
    fragments, k = components_ref.components(aff, fragment_threshold, 0)
    edges, counts, sums, sizes = region_graph(fragments, aff, k)
    table, _ = agglomerate(edges, counts, sums, sizes, thresholds[-1], min_segment_size)
    return table[fragments]
