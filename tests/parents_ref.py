"""
CPU oracles of geodesic_parents and trace_paths (exaspim_geodesic_parents_begin / _sweeps / _finish,
exaspim_trace_paths), written from the definition, and the volumes the CPU and GPU tests share.

The definition: labels, sources, cost, adjacency, K and the weights w(u -> v) are geodesic_ref.py's; d is the
converged field of exactly these inputs. A source row is valid iff it names a voxel of its label whose field
word is +0.0. An edge u -> v is tight iff u and v are adjacent, d[u] and d[v] are finite, v is not its label's
source, and fl32(d[u] + w(u -> v)) has the bit pattern of d[v]. hops h (int32) is the least solution of
h[source] = 0, h[v] = 1 + min over tight u -> v of h[u]; parent[source] = the source's own index, otherwise the
tight predecessor u with h[u] = h[v] - 1 that has the smallest C-order index. Everything else gets h = -1 and
parent = -1. An orphan is a voxel of a label in 1..K with finite d that is no source and has no tight
predecessor.

  breadth_first  oracle (a): a breadth-first search over tight edges and the parent rule, in plain Python.
  jacobi         oracle (b): rounds of 26 shifted numpy arrays over the tight masks to the fixed point.
  walk           the path of a target, read off parents.
"""

import collections

import numpy as np

import geodesic_ref as ref

OFFSETS = ref.OFFSETS      # in the order of the C-order linear index: (dz, dy, dx) ascending


def valid_sources(labels, sources, field):
    """(sources with the invalid rows set to -1, the number of invalid rows): a source's field word must be +0.0."""
    out, invalid = ref.valid_sources(labels, sources)
    words = ref.bits(np.asarray(field, dtype=np.float32)).reshape(-1)
    for row in range(1, len(out)):
        if out[row] >= 0 and words[out[row]] != 0:
            out[row] = -1
            invalid += 1
    return out, invalid


def _start(labels, sources, field):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    field = np.ascontiguousarray(field, dtype=np.float32)
    assert labels.ndim == 3 and field.shape == labels.shape
    k = len(sources) - 1
    sources, invalid = valid_sources(labels, sources, field)
    joined = np.where((labels >= 1) & (labels <= k) & np.isfinite(field), labels, 0)   # what takes part in tight edges
    hops = np.full(labels.shape, -1, dtype=np.int32)
    for row in range(1, k + 1):
        if sources[row] >= 0:
            hops.reshape(-1)[sources[row]] = 0
    return labels, field, sources, invalid, joined, hops


def _sum_bits(a, b):
    """The bit pattern of the one float32 addition a + b."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)).astype(np.float32).view(np.int32)


def breadth_first(labels, sources, field, cost=None):
    """Oracle (a): (parents int32, hops int32, orphans, invalid rows)."""
    labels, field, sources, invalid, joined, hops = _start(labels, sources, field)
    shape = labels.shape
    w = None if cost is None else ref.entering_weight(cost)
    words = ref.bits(field)
    is_source = hops == 0

    def neighbours(v):
        for o in OFFSETS:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if min(u) >= 0 and all(c < s for c, s in zip(u, shape)) and joined[u] == joined[v]:
                yield u, o

    def tight(u, v, o):      # u -> v, both joined and of one label
        if is_source[v]:
            return False
        step = ref.STEP[sum(c != 0 for c in o)] if w is None else w[v]
        return int(_sum_bits(field[u], step)) == int(words[v])

    queue = collections.deque(tuple(int(c) for c in np.unravel_index(s, shape)) for s in sources[1:] if s >= 0)
    while queue:
        u = queue.popleft()
        for v, o in neighbours(u):
            if hops[v] < 0 and tight(u, v, o):
                hops[v] = hops[u] + 1
                queue.append(v)
    parents = np.full(shape, -1, dtype=np.int32)
    orphans = 0
    for v in zip(*np.nonzero(joined)):
        index = int(np.ravel_multi_index(v, shape))
        if is_source[v]:
            parents[v] = index
            continue
        before = [u for u, o in neighbours(v) if tight(u, v, o)]      # in the order of the linear index
        if not before:
            orphans += 1
        for u in before:
            if hops[v] >= 1 and hops[u] == hops[v] - 1:
                parents[v] = int(np.ravel_multi_index(u, shape))
                break
    return parents, hops, orphans, invalid


def jacobi(labels, sources, field, cost=None, return_rounds=False):
    """Oracle (b): (parents int32, hops int32, orphans, invalid rows), by rounds of 26 shifted arrays."""
    labels, field, sources, invalid, joined, hops = _start(labels, sources, field)
    shape = labels.shape
    parents = np.full(shape, -1, dtype=np.int32)
    orphans = rounds = 0
    if joined.any():
        big = np.int64(1) << 40
        box = tuple(slice(int(idx.min()), int(idx.max()) + 1) for idx in np.nonzero(joined))
        lab = np.pad(joined[box], 1)
        d = np.pad(field[box], 1, constant_values=ref.INF)
        index = np.pad(np.arange(labels.size, dtype=np.int64).reshape(shape)[box], 1, constant_values=-1)
        h = np.pad(np.where(hops[box] == 0, np.int64(0), big), 1, constant_values=big)
        w = None if cost is None else ref.entering_weight(cost)[box]
        inner = (slice(1, -1),) * 3
        me, mine, source = lab[inner], d[inner].view(np.int32), h[inner] == 0
        links = []      # (the shifted slice, where its edge into the inner voxel is tight)
        any_tight = np.zeros(me.shape, dtype=bool)
        for o in OFFSETS:
            sl = tuple(slice(1 + c, lab.shape[a] - 1 + c) for a, c in enumerate(o))
            step = ref.STEP[sum(c != 0 for c in o)] if w is None else w
            is_tight = (lab[sl] == me) & (me > 0) & ~source & (_sum_bits(d[sl], step) == mine)
            any_tight |= is_tight
            if is_tight.any():
                links.append((sl, is_tight))
        while True:
            rounds += 1
            best = h[inner].copy()
            for sl, is_tight in links:
                np.minimum(best, np.where(is_tight, h[sl] + 1, big), out=best)
            if np.array_equal(best, h[inner]):
                break
            h[inner] = best
        reached = (h[inner] < big) & (me > 0)
        hops[box] = np.where(reached, h[inner], -1).astype(np.int32)
        chosen = np.where(source, index[inner], -1)
        for sl, is_tight in reversed(links):      # the smallest index is written last
            chosen = np.where(is_tight & reached & (h[sl] == h[inner] - 1), index[sl], chosen)
        parents[box] = chosen.astype(np.int32)
        orphans = int(((me > 0) & ~source & ~any_tight).sum())
    out = (parents, hops, orphans, invalid)
    return out + (rounds,) if return_rounds else out


def walk(parents, hops, target):
    """The path of "target", source first: hops[target] + 1 linear indices."""
    parents, hops = parents.reshape(-1), hops.reshape(-1)
    h = int(hops[target])
    assert h >= 0
    path = [int(target)]
    for _ in range(h):
        path.append(int(parents[path[-1]]))
        assert path[-1] >= 0
    assert parents[path[-1]] == path[-1]      # the walk ends on a source
    return path[::-1]


def paths(parents, hops, targets):
    """(voxels int32 (N,), offsets int64 (T + 1,)) of trace_paths."""
    rows = [walk(parents, hops, int(t)) for t in targets]
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.array([v for r in rows for v in r], dtype=np.int32), offsets


# ---- volumes -----------------------------------------------------------------------------------------
BIG = np.float32(2.0 ** 25)      # fl32(2^25 + 1) = 2^25: a cost of 1 is absorbed


def absorbed_case(seed):
    """seeded_case(seed) of an odd seed with its cost scaled by 3e7 and 1e-3 entries mixed in: costs are absorbed."""
    assert seed % 2 == 1
    labels, sources, cost = ref.seeded_case(seed)
    rng = np.random.default_rng(7000 + seed)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (cost * np.float32(3e7)).astype(np.float32)
    return labels, sources, np.where(rng.random(cost.shape) < 0.3, np.float32(1e-3), scaled).astype(np.float32)


def plateau_line(n=70):
    """A line along x of n voxels, the source at its +x end, 2^25 next to it and 1 elsewhere: one plateau of 2^25."""
    shape = (3, 3, n)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 1, :] = 1
    cost = np.ones(shape, dtype=np.float32)
    cost[:, :, n - 2] = BIG
    sources = np.array([-1, np.ravel_multi_index((1, 1, n - 1), shape)], dtype=np.int32)
    return labels, sources, cost


def plateau_slab(shape=(3, 12, 40)):
    """A full slab with the same plateau: the plane next to the source's costs 2^25."""
    labels = np.ones(shape, dtype=np.int32)
    cost = np.ones(shape, dtype=np.float32)
    cost[:, :, shape[2] - 2] = BIG
    sources = np.array([-1, np.ravel_multi_index((1, 5, shape[2] - 1), shape)], dtype=np.int32)
    return labels, sources, cost


def plateau_count(parents, field):
    """Voxels whose parent is another voxel with the same field bits: where only hops keep the chain acyclic."""
    flat, words = parents.reshape(-1), ref.bits(field).reshape(-1)
    v = np.nonzero((flat >= 0) & (flat != np.arange(flat.size)))[0]
    return int((words[flat[v]] == words[v]).sum())
