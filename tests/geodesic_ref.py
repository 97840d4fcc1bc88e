"""
CPU oracles of geodesic_field (exaspim_geodesic_begin / _sweeps / _farthest), written from the
definition, and the volumes the CPU and GPU tests share.

The definition: labels <= 0 is background; K = len(sources) - 1; sources[L] is the C-order linear index of
label L's source, -1 for none, row 0 ignored; a row is valid iff it names a voxel of its label. Two voxels
are adjacent iff they differ by at most 1 in every coordinate, are not equal and carry the same label in
1..K. A step costs 1.0f, 0x3FB504F3 or 0x3FDDB3D7 by the number of coordinates that differ (Euclidean mode)
or the float32 cost of the voxel entered (cost mode: -0.0 is 0; negative, NaN and +inf cannot be entered).
d is the least solution of d[source] = 0, d[v] = min over adjacent u of fl32(d[u] + w(u -> v)). Background
gets 0.0; foreground that is not reached gets +inf.

  heap_dijkstra  one heap Dijkstra per label, every sum a numpy.float32 addition.
  relaxation     26 shifted float32 arrays, repeated to the fixed point (on the foreground's bounding box).
  farthest       per label the largest finite value and the smallest C-order index attaining it.
"""

import heapq
import itertools

import numpy as np

SQRT2 = np.array([0x3FB504F3], dtype=np.uint32).view(np.float32)[0]
SQRT3 = np.array([0x3FDDB3D7], dtype=np.uint32).view(np.float32)[0]
STEP = {1: np.float32(1.0), 2: SQRT2, 3: SQRT3}
OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
INF = np.float32(np.inf)


def bits(field):
    """The int32 bit patterns of a float32 array: what every comparison of two fields is made on."""
    field = np.ascontiguousarray(field)
    assert field.dtype == np.float32
    return field.view(np.int32)


def valid_sources(labels, sources):
    """(sources with the invalid rows set to -1, the number of invalid rows)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    flat = labels.reshape(-1)
    out = np.array(sources, dtype=np.int64)
    invalid = 0
    out[0] = -1
    for row in range(1, len(out)):
        s = out[row]
        if s == -1:
            continue
        if not (0 <= s < flat.size and flat[s] == row):
            out[row] = -1
            invalid += 1
    return out, invalid


def entering_weight(cost):
    """The float32 weight of entering each voxel in cost mode."""
    cost = np.asarray(cost, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(cost >= 0, np.abs(cost), INF).astype(np.float32)


def _start(labels, sources):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    assert labels.ndim == 3
    k = len(sources) - 1
    sources, _ = valid_sources(labels, sources)
    d = np.where(labels > 0, INF, np.float32(0)).astype(np.float32)
    for row in range(1, k + 1):
        if sources[row] >= 0:
            d.reshape(-1)[sources[row]] = 0
    joined = np.where((labels >= 1) & (labels <= k), labels, 0)     # what takes part in the graph
    return labels, sources, d, joined


def heap_dijkstra(labels, sources, cost=None):
    """Oracle (a): float32 (D, H, W)."""
    labels, sources, d, joined = _start(labels, sources)
    shape = labels.shape
    w = None if cost is None else entering_weight(cost)
    for row in range(1, len(sources)):
        if sources[row] < 0:
            continue
        start = tuple(int(c) for c in np.unravel_index(sources[row], shape))
        heap = [(np.float32(0), start)]
        done = set()
        while heap:
            du, u = heapq.heappop(heap)
            if u in done:
                continue
            done.add(u)
            for o in OFFSETS:
                v = (u[0] + o[0], u[1] + o[1], u[2] + o[2])
                if min(v) < 0 or any(c >= s for c, s in zip(v, shape)) or joined[v] != row or v in done:
                    continue
                step = STEP[sum(c != 0 for c in o)] if w is None else w[v]
                dv = np.float32(du + step)      # one float32 addition
                if dv < d[v]:
                    d[v] = dv
                    heapq.heappush(heap, (dv, v))
    return d


def relaxation(labels, sources, cost=None, return_rounds=False):
    """Oracle (b): float32 (D, H, W), by Jacobi rounds of 26 shifted arrays."""
    labels, sources, d, joined = _start(labels, sources)
    rounds = 0
    if joined.any():
        box = tuple(slice(int(idx.min()), int(idx.max()) + 1) for idx in np.nonzero(joined))
        lab = np.pad(joined[box], 1)
        cur = np.pad(d[box], 1, constant_values=INF)
        w = None if cost is None else np.pad(entering_weight(cost)[box], 1, constant_values=INF)
        inner = (slice(1, -1),) * 3
        me = lab[inner]
        links = []
        for o in OFFSETS:
            sl = tuple(slice(1 + c, lab.shape[a] - 1 + c) for a, c in enumerate(o))
            same = (lab[sl] == me) & (me > 0)
            if same.any():
                links.append((sl, same, STEP[sum(c != 0 for c in o)] if w is None else w[inner]))
        while True:
            rounds += 1
            best = cur[inner].copy()
            for sl, same, step in links:
                cand = (cur[sl] + step).astype(np.float32)      # float32 + float32: one rounded addition
                np.minimum(best, np.where(same, cand, INF), out=best)
            if np.array_equal(best.view(np.int32), cur[inner].view(np.int32)):
                break
            cur[inner] = best
        d[box] = cur[inner]
    return (d, rounds) if return_rounds else d


def farthest(labels, sources, field):
    """(far_value float32 (K + 1,), far_index int32 (K + 1,))."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    field = np.ascontiguousarray(field, dtype=np.float32).reshape(-1)
    sources, _ = valid_sources(labels, sources)
    k = len(sources) - 1
    value = np.zeros(k + 1, dtype=np.float32)
    index = np.full(k + 1, -1, dtype=np.int32)
    for row in range(1, k + 1):
        if sources[row] < 0:
            continue
        where = np.nonzero((labels == row) & np.isfinite(field))[0]
        value[row] = field[where].max()
        index[row] = where[field[where] == value[row]].min()
    return value, index


# ---- volumes -----------------------------------------------------------------------------------------
def first_voxels(labels, k):
    """Each label's first voxel in C order, -1 for an absent label: segment_table's peak_index without a field."""
    flat = np.asarray(labels).reshape(-1)
    out = np.full(k + 1, -1, dtype=np.int32)
    for row in range(1, k + 1):
        where = np.nonzero(flat == row)[0]
        if where.size:
            out[row] = where[0]
    return out


def random_sources(rng, labels, k):
    """A random voxel of each present label."""
    flat = np.asarray(labels).reshape(-1)
    out = np.full(k + 1, -1, dtype=np.int32)
    for row in range(1, k + 1):
        where = np.nonzero(flat == row)[0]
        if where.size:
            out[row] = rng.choice(where)
    return out


def blobs(rng, shape, n_labels, fill=0.75):
    """Blob labels 1..n_labels around random centres, with voxels knocked out so that paths wind."""
    grid = np.indices(shape).reshape(3, -1).T
    centres = np.stack([rng.integers(0, s, n_labels) for s in shape], axis=1)
    dist = ((grid[:, None, :] - centres[None]) ** 2).sum(-1)
    radius = max(2.0, 0.45 * min(max(shape), 14))
    labels = np.where(dist.min(1) <= radius ** 2, dist.argmin(1) + 1, 0).astype(np.int32).reshape(shape)
    labels[rng.random(shape) > fill] = 0
    return labels


def random_cost(rng, shape):
    """Costs with exact ties and every special value: 0, -0.0, +inf, NaN, negatives, tiny and large."""
    cost = rng.choice(np.array([0.25, 0.5, 1.0, 1.5, 3.0, 1e-3, 1e4], dtype=np.float32), size=shape)
    cost = (cost + (rng.random(shape) < 0.3) * rng.random(shape).astype(np.float32)).astype(np.float32)
    special = rng.random(shape)
    for lo, value in ((0.00, 0.0), (0.04, -0.0), (0.08, np.inf), (0.10, np.nan), (0.12, -1.0), (0.14, -np.inf)):
        cost[(special >= lo) & (special < lo + (0.04 if lo < 0.08 else 0.02))] = value
    return cost.astype(np.float32)


def seeded_case(seed, max_shape=(10, 10, 10), max_labels=4, shape=None):
    """(labels, sources, cost or None) of one seed; odd seeds are in cost mode. "shape" overrides the drawn one."""
    rng = np.random.default_rng(9000 + seed)
    drawn = tuple(int(rng.integers(1, m + 1)) for m in max_shape)
    shape = drawn if shape is None else shape
    k = int(rng.integers(1, max_labels + 1))
    labels = blobs(rng, shape, k)
    if seed % 5 == 0:
        labels[rng.random(shape) < 0.05] = k + 2      # a label above K
        labels[rng.random(shape) < 0.05] = -3
    sources = random_sources(rng, labels, k)
    if seed % 7 == 3 and k > 1:
        sources[k] = -1
    cost = random_cost(rng, shape) if seed % 2 else None
    return labels, sources, cost


def serpentine(shape=(16, 16, 64), z=3, label=1):
    """A one-voxel-wide path in the plane z: every other row in full, joined at alternating ends."""
    labels = np.zeros(shape, dtype=np.int32)
    for i, y in enumerate(range(0, shape[1], 2)):
        labels[z, y, :] = label
        if y + 2 < shape[1]:
            labels[z, y + 1, shape[2] - 1 if i % 2 == 0 else 0] = label
    return labels
