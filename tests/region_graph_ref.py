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
    agglomerate_fast(edges, counts, sums, sizes, threshold, min_size)
                                    -> agglomerate's (table, S) with a heap, for graphs of 10^4 fragments;
                                       agglomerate stays the definition
    mean_graph(seed, k, n_edges), wide_graph(seed, k, n_edges, levels, count_max, total_max, hubs)
                                    -> random graphs (edges, counts, sums, sizes) for the tests
    fragment_volume(kind, dtype), stride_volume(dtype)
                                    -> volumes with their oracles, shared by the GPU tests: 10^4 fragments;
                                       more than twice the tiles of one capped launch
"""

import heapq

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


class _Best:
    """Heap entry of agglomerate_fast: the larger exact mean sorts first, then the smaller (lo, hi)."""

    __slots__ = ("count", "sum", "lo", "hi")

    def __init__(self, count, total, lo, hi):
        self.count, self.sum, self.lo, self.hi = count, total, lo, hi

    def __lt__(self, other):
        left, right = self.sum * other.count, other.sum * self.count      # Python ints: exact at any width
        if left != right:
            return left > right
        return (self.lo, self.hi) < (other.lo, other.hi)


def agglomerate_fast(edges, counts, sums, sizes, threshold, min_size, merges=None):
    """
    agglomerate's contract in O(E log E) for the graphs the naive scan cannot reach; trusted only because
    tests/test_agglomerate_scale_cpu.py holds it to agglomerate on small graphs. near[r] maps each current
    neighbour root of root r to the contact's (count, sum); a heap entry is valid iff near[lo] still holds
    its (count, sum) under hi. A merge moves the larger id's neighbours under the smaller id, pooling the
    ones both have. "merges", a list, receives (lo, hi) of every merge in order.
    """
    k = len(sizes) - 1
    m = int(np.rint((1.0 - float(np.float32(threshold))) * ONE))
    near = {r: {} for r in range(k + 1)}        # one dict per current root id
    heap = []
    for (lo, hi), c, s in zip(np.asarray(edges).tolist(), np.asarray(counts).tolist(), np.asarray(sums).tolist()):
        near[lo][hi] = near[hi][lo] = (c, s)
        heap.append(_Best(c, s, lo, hi))
    heapq.heapify(heap)
    root = list(range(k + 1))
    while heap:
        top = heapq.heappop(heap)
        u, v = top.lo, top.hi
        if u not in near or near[u].get(v) != (top.count, top.sum):
            continue
        if not top.sum > m * top.count:
            break
        if merges is not None:
            merges.append((u, v))
        del near[u][v], near[v][u]
        root[v] = u
        for w, (c, s) in near[v].items():
            del near[w][v]
            if w in near[u]:
                c, s = c + near[u][w][0], s + near[u][w][1]
            near[u][w] = near[w][u] = (c, s)
            heapq.heappush(heap, _Best(c, s, min(u, w), max(u, w)))
        del near[v]
    total = [0] * (k + 1)
    for label in range(1, k + 1):      # root[v] < v, so root[root[label]] is final when label comes
        root[label] = root[root[label]]
        total[root[label]] += int(sizes[label])
    table = np.zeros(k + 1, np.int32)
    count = 0
    for label in range(1, k + 1):
        if root[label] == label:
            if total[label] > min_size:
                count += 1
                table[label] = count
        else:
            table[label] = table[root[label]]
    return table, count


def _distinct_pairs(rng, k, n_edges, hubs=None):
    """About n_edges distinct pairs lo < hi in 1 .. k, sorted; hubs=(n, degree) adds n stars of that degree."""
    a = rng.integers(1, k + 1, n_edges)
    b = rng.integers(1, k + 1, n_edges)
    if hubs is not None:
        n, degree = hubs
        for hub in rng.choice(np.arange(1, k + 1), n, replace=False):
            a = np.concatenate([a, np.full(degree, hub)])
            b = np.concatenate([b, rng.choice(np.arange(1, k + 1), degree, replace=False)])
    keep = a != b
    keys = np.unique((np.minimum(a, b)[keep].astype(np.int64) << 32) | np.maximum(a, b)[keep])
    return np.stack([keys >> 32, keys & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)


def mean_graph(seed, k, n_edges, count_max=49, max_size=40):
    """A random graph with arbitrary means: counts 1 .. count_max, sums uniform in 0 .. count * 2^24."""
    rng = np.random.default_rng(seed)
    edges = _distinct_pairs(rng, k, n_edges)
    counts = rng.integers(1, count_max + 1, len(edges)).astype(np.int64)
    sums = rng.integers(0, counts * ONE + 1).astype(np.uint64)
    return edges, counts, sums, rng.integers(1, max_size + 1, k + 1).astype(np.int64)


def wide_graph(seed, k, n_edges, levels, count_max, total_max=1 << 39, hubs=None, max_size=40):
    """
    A random graph of near-ties between wide operands: about n_edges distinct pairs (plus the stars of
    hubs=(n, degree)), counts uniform in 1 .. count_max but 1 once the running total would pass total_max,
    sum = count * level + delta clamped to 0 .. count * 2^24, with level one of "levels" equally spaced
    values of 0 .. 2^24 and delta in {-1, 0, 1}. With count_max near 2^34 the cross products of two
    edges need more than 64 bits, and two means differ by far less than a double resolves.
    """
    rng = np.random.default_rng(seed)
    edges = _distinct_pairs(rng, k, n_edges, hubs)
    drawn = rng.integers(1, count_max + 1, len(edges)).tolist()
    step = ONE // (levels - 1)
    level = (rng.integers(0, levels, len(edges)) * step).tolist()
    delta = rng.integers(-1, 2, len(edges)).tolist()
    counts, sums, total = [], [], 0
    for i, (c, q, d) in enumerate(zip(drawn, level, delta)):
        if total + c + (len(drawn) - 1 - i) > total_max:     # the edges still to come count at least 1 each
            c = 1
        total += c
        counts.append(c)
        sums.append(min(max(c * q + d, 0), c * ONE))
    return (edges, np.array(counts, np.int64).reshape(-1), np.array(sums, np.uint64).reshape(-1),
            rng.integers(1, max_size + 1, k + 1).astype(np.int64))


_VOLUMES = {}


def fragment_volume(kind, dtype=np.float32, shape=(33, 65, 129)):
    """
    (aff, fragments, K, graph) of uniform random affinities with some 10^4 fragments, computed once per
    session and read-only: kind "watershed" (basins between 0.3 and 0.7) or "components" (cut at 0.75).
    """
    import watershed_ref

    key = (kind, np.dtype(dtype).name, tuple(shape))
    if key not in _VOLUMES:
        aff = np.array(watershed_ref.random_affinities("uniform", shape)).astype(dtype)
        if kind == "watershed":
            fragments, k = watershed_ref.fragments(aff, 0.3, 0.7)
        else:
            fragments, k = components_ref.components(aff, 0.75, 0)
        graph = region_graph(fragments, aff, k)
        for a in (aff, fragments) + graph:
            a.setflags(write=False)
        _VOLUMES[key] = (aff, fragments, k, graph)
    return _VOLUMES[key]


STRIDE_SHAPE = (8 * 73728, 9, 2)      # 73728 * 2 * 1 = 147 456 tiles of 8 x 8 x 32, 10.6M voxels
STRIDE_FIRST_TRIP = 65536             # workgroups of one capped launch: the tiles of every workgroup's first trip


def stride_volume(dtype=np.float32):
    """
    (labels, aff, K, graph, behind) of a long thin volume with more than twice the tiles one capped launch
    of tile_graph covers, so every workgroup makes two or three trips; computed once per session and
    read-only. The labels are slabs of random thickness 1 .. 23 along z, each with an id of its own and
    split in y at row 5 (the second tile row in y holds one voxel row), with 2 % of the voxels set to 0:
    some three edges per slab, the contact inside a slab with up to 46 voxel edges. behind is the oracle's
    graph of the planes behind the first STRIDE_FIRST_TRIP tiles alone (the tiles run along z here, two to
    a step of 8 planes).
    """
    key = ("stride", np.dtype(dtype).name)
    if key not in _VOLUMES:
        d, h, w = STRIDE_SHAPE
        rng = np.random.default_rng(47)
        thickness = rng.integers(1, 24, size=d)                  # more slabs than the volume can hold
        slab = np.repeat(np.arange(1, d + 1, dtype=np.int32), thickness)[:d]
        labels = np.repeat(slab * 2, h * w).reshape(STRIDE_SHAPE)
        labels[:, :5] -= 1
        labels[rng.random(STRIDE_SHAPE) < 0.02] = 0
        k = int(labels.max())
        aff = rng.random((3,) + STRIDE_SHAPE, dtype=np.float32).astype(dtype)
        graph = region_graph(labels, aff, k)
        z = STRIDE_FIRST_TRIP // (-(-h // 8) * -(-w // 32)) * 8
        behind = region_graph(labels[z:], aff[:, z:], k)
        for a in (labels, aff) + graph + behind:
            a.setflags(write=False)
        _VOLUMES[key] = (labels, aff, k, graph, behind)
    return _VOLUMES[key]


def agglomerate_affinities(aff, agglomeration_thresholds=(0.6, 0.8, 0.9), min_segment_size=100,
                           fragment_threshold=0.5):
    thresholds = list(agglomeration_thresholds)
    assert all(b >= a for a, b in zip(thresholds, thresholds[1:]))
    fragments, k = components_ref.components(aff, fragment_threshold, 0)
    edges, counts, sums, sizes = region_graph(fragments, aff, k)
    table, _ = agglomerate(edges, counts, sums, sizes, thresholds[-1], min_segment_size)
    return table[fragments]
