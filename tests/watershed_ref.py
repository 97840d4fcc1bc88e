"""
CPU oracles of exaspim_watershed_fragments (include/exaspim_affinity.h).

    fragments(aff, low, high, min_size) -> (labels int32 (D, H, W), K)

is written straight from the definition: aff is (3, D, H, W), float32 or float16 (widened exactly),
channel c at voxel v = edge v -- v + e_c, e = z, y, x, the last index along axis c ignored; low and
high are rounded to float32.
  1. An edge is eligible iff float32(a) > low (NaN never, +inf always).
  2. A voxel's steepest edge is its eligible incident edge of largest value; among equal values the
     first in the order -z, -y, -x, +x, +y, +z (the other end's C-order linear index).
  3. An eligible edge is on iff a >= high or it is the steepest edge of one of its two ends.
  4. Fragments are the connected components of the on edges, filtered and numbered by
     components_ref.components (kept iff size > max(min_size, 1), 1 .. K in raster order of the
     first voxel).

    serial_fragments(aff, low, high) -> (labels int32 (D, H, W), K)

is the serial steepest-ascent watershed in four steps, written from its description (Zlateski's, as
waterz runs it) in the project's edge convention: direction bits per voxel for "this edge is the
voxel's maximum, or >= high" where the maximum exceeds low; plateau corners (voxels with an edge
that is not answered); breadth-first division of the plateaus from the corners; pointer chasing
with ids given in raster order. It depends on its visiting order where a voxel has two equal
maximal edges below high; elsewhere it gives fragments()'s labels (tests/test_watershed_cpu.py).

    tied_voxels(aff, low, high) -> number of voxels with two equal maximal eligible edges below high

The inputs both test files share: random_affinities(kind, shape) and the hand-built lines LINES with
line_affinities(axis, values).
"""

import numpy as np

import components_ref

# direction d = 0 .. 5: (axis, sign) in the order of the other end's linear index
DIRECTIONS = ((0, -1), (1, -1), (2, -1), (2, +1), (1, +1), (0, +1))


def _as_float32(aff):
    aff = np.asarray(aff)
    if aff.dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise TypeError(aff.dtype)
    if aff.ndim != 4 or aff.shape[0] != 3:
        raise ValueError(aff.shape)
    return aff.astype(np.float32)


def incident(aff):
    """(6, D, H, W) float32: the value of every voxel's edge in direction d, NaN where it leaves the volume."""
    a = _as_float32(aff)
    out = np.full((6,) + a.shape[1:], np.nan, np.float32)
    for d, (axis, sign) in enumerate(DIRECTIONS):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        if sign > 0:
            out[d][tuple(lo)] = a[axis][tuple(lo)]
        else:
            out[d][tuple(hi)] = a[axis][tuple(lo)]
    return out


def steepest(aff, low):
    """int8 (D, H, W): 0 where a voxel has no eligible edge, else 1 + the direction of its steepest one."""
    inc = incident(aff)
    with np.errstate(invalid="ignore"):
        eligible = inc > np.float32(low)
    value = np.where(eligible, inc, -np.inf)
    code = value.argmax(axis=0) + 1      # argmax takes the first of equal values
    return np.where(eligible.any(axis=0), code, 0).astype(np.int8)


def on_edges(aff, low, high):
    """(on_z, on_y, on_x): boolean (D, H, W), edge c of voxel v joins v and v + e_c."""
    a = _as_float32(aff)
    low, high = np.float32(low), np.float32(high)
    code = steepest(a, low)
    on = []
    for axis in range(3):
        up = 1 + DIRECTIONS.index((axis, +1))
        down = 1 + DIRECTIONS.index((axis, -1))
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        e = np.zeros(a.shape[1:], bool)
        with np.errstate(invalid="ignore"):
            eligible = a[axis][lo] > low
            e[lo] = eligible & ((a[axis][lo] >= high) | (code[lo] == up) | (code[hi] == down))
        on.append(e)
    return tuple(on)


def fragments(aff, low=0.1, high=0.9999, min_size=0):
    on = on_edges(aff, low, high)
    return components_ref.components(np.stack(on).astype(np.float32), 0.5, min_size)


def tied_voxels(aff, low, high):
    inc = incident(aff)
    with np.errstate(invalid="ignore"):
        eligible = inc > np.float32(low)
    value = np.where(eligible, inc, -np.inf)
    top = value.max(axis=0)
    tied = ((value == top) & eligible).sum(axis=0) >= 2
    return int((tied & (top < np.float32(high))).sum())


def serial_fragments(aff, low=0.1, high=0.9999):
    a = _as_float32(aff)
    low, high = np.float32(low), np.float32(high)
    shape = a.shape[1:]
    n = int(np.prod(shape))
    strides = (shape[1] * shape[2], shape[2], 1)
    step = [sign * strides[axis] for axis, sign in DIRECTIONS]
    opposite = [5, 4, 3, 2, 1, 0]
    visited = 0x40

    # 1. direction bits: edge d of v is v's maximum or >= high, where the maximum exceeds low
    inc = incident(a)
    with np.errstate(invalid="ignore"):
        eligible = inc > low
        top = np.where(eligible, inc, -np.inf).max(axis=0)
        bit = eligible & ((inc == top) | (inc >= high))
    seg = np.zeros(shape, np.int64)
    for d in range(6):
        seg |= bit[d].astype(np.int64) << d
    seg = seg.ravel().tolist()

    # 2. plateau corners: voxels with an edge the other end does not answer
    queue = []
    for v in range(n):
        s = seg[v]
        for d in range(6):
            if s >> d & 1 and not seg[v + step[d]] >> opposite[d] & 1:
                seg[v] |= visited
                queue.append(v)
                break

    # 3. divide the plateaus breadth first: every reached voxel keeps one edge out
    head = 0
    while head < len(queue):
        v = queue[head]
        head += 1
        keep = 0
        s = seg[v]
        for d in range(6):
            if s >> d & 1:
                u = v + step[d]
                if seg[u] >> opposite[d] & 1:
                    if not seg[u] & visited:
                        seg[u] |= visited
                        queue.append(u)
                else:
                    keep = 1 << d
        seg[v] = keep | visited

    # 4. chase the pointers, ids in raster order
    label = [0] * n
    seen = [False] * n
    next_id = 1
    for v in range(n):
        if not seg[v] & 0x3F or label[v]:
            continue
        chain = [v]
        seen[v] = True
        found = 0
        head = 0
        while head < len(chain) and not found:
            me = chain[head]
            head += 1
            for d in range(6):
                if seg[me] >> d & 1:
                    him = me + step[d]
                    if label[him]:
                        found = label[him]
                        break
                    if not seen[him]:
                        seen[him] = True
                        chain.append(him)
        if not found:
            found = next_id
            next_id += 1
        for u in chain:
            label[u] = found
    return np.array(label, np.int32).reshape(shape), next_id - 1


# ---- inputs the CPU and the GPU tests share -------------------------------------------------------------
SHAPES = [(5, 6, 7), (7, 5, 3), (8, 8, 32), (9, 9, 33), (16, 16, 64), (17, 17, 65), (12, 10, 20), (1, 1, 40),
          (3, 1, 5)]
THRESHOLDS = [(0.1, 0.9999), (0.3, 0.7), (0.0, 2.0), (-1.0, 2.0)]
_RANDOM = {}


def random_affinities(kind, shape, seed=7):
    """float32 (3,) + shape, read-only: "uniform", "smooth" (a 3 x 3 x 3 box mean) or "saturated"."""
    key = (kind, tuple(shape), seed)
    if key not in _RANDOM:
        u = np.random.default_rng(seed).random((3,) + tuple(shape)).astype(np.float32)
        if kind == "smooth":
            from scipy import ndimage

            u = ndimage.uniform_filter(u, size=(1, 3, 3, 3), mode="nearest").astype(np.float32)
        elif kind == "saturated":
            u = np.clip(np.float32(1.5) * u - np.float32(0.1), 0, 1).astype(np.float32)
        elif kind != "uniform":
            raise ValueError(kind)
        u.setflags(write=False)
        _RANDOM[key] = u
    return _RANDOM[key]


def line_affinities(axis, values):
    """
    A line of len(values) voxels along "axis": channel "axis" holds the values (the last one leaves the
    volume), the other two channels, whose every entry leaves the volume, hold 1.
    """
    shape = [1, 1, 1]
    shape[axis] = len(values)
    aff = np.ones((3,) + tuple(shape), np.float32)
    aff[axis] = np.asarray(values, np.float32).reshape(shape)
    return aff


_LOW, _HIGH = np.float32(0.1), np.float32(0.3)
_INF, _NAN = np.float32(np.inf), np.float32(np.nan)
# (name, values along the line, low, high, min_size, labels)
LINES = [
    ("eligible but off", [0.5, 0.2, 0.6, 1.0], 0.1, 0.9999, 0, [1, 1, 2, 2]),
    ("high below the saddle", [0.5, 0.2, 0.6, 1.0], 0.1, 0.15, 0, [1, 1, 1, 1]),
    ("background at both ends", [0.05, 0.5, 0.05, 1.0], 0.1, 0.9999, 0, [0, 1, 1, 0]),
    ("a == low is off", [0.5, _LOW, 0.6, 1.0], _LOW, 0.05, 0, [1, 1, 2, 2]),
    ("a just above low is eligible", [0.5, _LOW, 0.6, 1.0], np.nextafter(_LOW, np.float32(0)), 0.05, 0,
     [1, 1, 1, 1]),
    ("all edges == low", [_LOW, _LOW, _LOW, 1.0], _LOW, 0.05, 0, [0, 0, 0, 0]),
    ("a == high is on", [0.5, _HIGH, 0.6, 1.0], 0.1, _HIGH, 0, [1, 1, 1, 1]),
    ("a just below high is off", [0.5, _HIGH, 0.6, 1.0], 0.1, np.nextafter(_HIGH, np.float32(1)), 0,
     [1, 1, 2, 2]),
    ("NaN is never eligible", [0.5, _NAN, 0.6, 1.0], -1.0, -2.0, 0, [1, 1, 2, 2]),
    ("NaN alone", [_NAN, _NAN, 1.0], -1.0, -2.0, 0, [0, 0, 0]),
    ("+inf is on", [0.5, _INF, 0.6, 1.0], 0.1, 0.9999, 0, [1, 1, 1, 1]),
    ("+inf with high = +inf", [_INF, 0.5, 1.0], 0.1, _INF, 0, [1, 1, 1]),
    ("-inf with low = -inf", [0.5, -_INF, 0.6, 1.0], -_INF, -_INF, 0, [1, 1, 2, 2]),
    ("tie: the lower neighbour wins", [0.9, 0.5, 0.5, 0.9, 1.0], 0.1, 0.9999, 0, [1, 1, 1, 2, 2]),
    ("numbering by first voxel", [0.05, 0.5, 0.05, 0.5, 1.0], 0.1, 0.9999, 0, [0, 1, 1, 2, 2]),
    ("min_size 0", [0.5, 0.05, 0.5, 0.5, 0.05, 1.0], 0.1, 0.9999, 0, [1, 1, 2, 2, 2, 0]),
    ("min_size below the floor of 1", [0.5, 0.05, 0.5, 0.5, 0.05, 1.0], 0.1, 0.9999, -5, [1, 1, 2, 2, 2, 0]),
    ("min_size 1", [0.5, 0.05, 0.5, 0.5, 0.05, 1.0], 0.1, 0.9999, 1, [1, 1, 2, 2, 2, 0]),
    ("min_size 2", [0.5, 0.05, 0.5, 0.5, 0.05, 1.0], 0.1, 0.9999, 2, [0, 0, 1, 1, 1, 0]),
    ("min_size 3", [0.5, 0.05, 0.5, 0.5, 0.05, 1.0], 0.1, 0.9999, 3, [0, 0, 0, 0, 0, 0]),
]
