"""
CPU oracles of teasar_branches (exaspim_teasar_begin / _round / _apply), written from the
definition, and the volumes the CPU and GPU tests share.

The definition: K = len(sources) - 1. A voxel is eligible iff its label L is in 1..K, sources[L] names a voxel
of L, hops >= 0 and the bits of daf are below 0x7F800000. Round t: every label that still has a valid voxel
takes as target its valid voxel with the largest daf bits, ties to the smallest C-order index; the path is read
off parents; every voxel of the label inside the label's box within Chebyshev distance r(p) of a path voxel p
becomes invalid, r(p) = min(max(D, H, W), floor(float64(scale) * sqrt(float64(max(dbf[p], 0))) + float64(const))).

  whole_paths   the kimimaro-shaped form, in code of its own: every path goes to the root, a full cube is stamped
                around every voxel of it, and the round's new vertices are the path minus the earlier paths.
  incremental   the device's form: the walk stops at the junction with the skeleton, and every new vertex
                clears its cube minus the cube of the vertex before it (the junction for the first one).

Both return the state byte of every voxel after every round (bit 0 valid, bit 1 on the skeleton).
"""

import numpy as np

import geodesic_ref as ref

VALID, SKELETON = 1, 2
DBF_INF = 2**31 - 1


def radius(dbf_values, scale, const, cap):
    """int64 radii of squared distances: numpy's float64 product, sum and floor, then the cap."""
    d2 = np.maximum(np.asarray(dbf_values, dtype=np.int64), 0)
    with np.errstate(over="ignore"):
        r = np.floor(np.float64(scale) * np.sqrt(d2.astype(np.float64)) + np.float64(const))
    return np.minimum(np.float64(cap), r).astype(np.int64)


def eligible(labels, sources, hops, daf):
    """The voxels that are valid before round 1."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    k = len(sources) - 1
    good, _ = ref.valid_sources(labels, sources)
    rooted = np.zeros(k + 1, dtype=bool)
    rooted[1:] = good[1:] >= 0
    words = ref.bits(np.ascontiguousarray(daf, dtype=np.float32)).view(np.uint32)
    inside = (labels >= 1) & (labels <= k)
    return inside & rooted[np.where(inside, labels, 0)] & (np.asarray(hops) >= 0) & (words < 0x7F800000)


def boxes_of(labels, k):
    """segment_table's boxes: int32 (K + 1, 6), half-open, zeros for an absent label and row 0."""
    boxes = np.zeros((k + 1, 6), dtype=np.int32)
    for row in range(1, k + 1):
        where = np.nonzero(np.asarray(labels) == row)
        if where[0].size:
            boxes[row] = [w.min() for w in where] + [w.max() + 1 for w in where]
    return boxes


def _cube(shape, box, v, r):
    """The slices of the cube of radius r around linear index v, clipped to the volume and the box; None if empty."""
    c = np.unravel_index(int(v), shape)
    lo = [max(int(c[a]) - int(r), int(box[a]), 0) for a in range(3)]
    hi = [min(int(c[a]) + int(r) + 1, int(box[3 + a]), shape[a]) for a in range(3)]
    if any(h <= l for l, h in zip(lo, hi)):
        return None
    return tuple(slice(l, h) for l, h in zip(lo, hi))


def _targets(labels, valid, words, k):
    """Per label the valid voxel with the largest daf bits and the smallest index, -1 without one."""
    flat_l, flat_v, flat_w = labels.reshape(-1), valid.reshape(-1), words.reshape(-1)
    out = np.full(k + 1, -1, dtype=np.int64)
    where = np.nonzero(flat_v)[0]
    for row in np.unique(flat_l[where]):
        mine = where[flat_l[where] == row]
        top = flat_w[mine].max()
        out[row] = mine[flat_w[mine] == top].min()
    return out


def _walk(parents, hops, skeleton, target, n):
    """
    The walk from "target" along parents, at most hops[target] steps, every index range-checked: (the walked
    voxels target first without the junction, the junction or -1), or None for a broken walk.
    """
    h = int(hops[target])
    if h < 0:
        return None
    cur, out = int(target), []
    for k in range(h, -1, -1):
        if skeleton[cur]:
            return out, cur
        out.append(cur)
        p = int(parents[cur])
        if k == 0:
            return (out, -1) if p == cur else None
        if p < 0 or p >= n or p == cur:
            return None
        cur = p
    raise AssertionError


class Result:
    """What one oracle run leaves: the per-round states and the branches in the device's order."""

    def __init__(self):
        self.states = []          # uint8 (D, H, W) after every round
        self.voxels, self.radii, self.before = [], [], []
        self.offsets = [0]
        self.branch_label, self.branch_round, self.branch_junction = [], [], []
        self.live, self.new, self.broken = [], [], 0

    def arrays(self):
        return (np.array(self.voxels, dtype=np.int32), np.array(self.radii, dtype=np.int32),
                np.array(self.offsets, dtype=np.int64), np.array(self.branch_label, dtype=np.int32),
                np.array(self.branch_round, dtype=np.int32), np.array(self.branch_junction, dtype=np.int32))

    def vertex_sets(self, k):
        """Per label the set of skeleton vertices."""
        sets = [set() for _ in range(k + 1)]
        for b, row in enumerate(self.branch_label):
            sets[row].update(self.voxels[self.offsets[b]:self.offsets[b + 1]])
        return sets


def _run(labels, sources, dbf, daf, parents, hops, scale, const, boxes, max_paths):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    shape, n, k = labels.shape, labels.size, len(sources) - 1
    if boxes is None:
        boxes = boxes_of(labels, k)
    cap = max(shape)
    flat_dbf = np.asarray(dbf).reshape(-1)
    flat_parents, flat_hops = np.asarray(parents).reshape(-1), np.asarray(hops).reshape(-1)
    words = ref.bits(np.ascontiguousarray(daf, dtype=np.float32)).view(np.uint32)
    valid = eligible(labels, sources, hops, daf)
    skeleton = np.zeros(shape, dtype=bool)
    flat_skel = skeleton.reshape(-1)
    finished = np.zeros(k + 1, dtype=bool)
    out = Result()
    rounds = 0
    while max_paths is None or rounds < max_paths:
        targets = _targets(labels, valid, words, k)
        live = [row for row in range(1, k + 1) if targets[row] >= 0 and not finished[row]]
        if not live:
            break
        rounds += 1
        n_live = n_new = 0
        for row in live:
            walked = _walk(flat_parents, flat_hops, flat_skel, targets[row], n)
            if walked is None:
                out.broken += 1
                finished[row] = True
                continue
            path, junction = walked
            fresh = path = path[::-1]      # ascending hops
            radii = radius(flat_dbf[path], scale, const, cap)
            mine = labels == row
            for i, (v, r) in enumerate(zip(path, radii)):
                cube = _cube(shape, boxes[row], v, r)
                if cube is None:
                    continue
                keep = np.zeros(shape, dtype=bool)      # the cube of the vertex before this one
                prev = path[i - 1] if i > 0 else junction
                if prev >= 0:
                    before = _cube(shape, boxes[row], prev, radius(flat_dbf[prev], scale, const, cap))
                    if before is not None:
                        keep[before] = True
                valid[cube] &= ~(mine[cube] & ~keep[cube])
            fresh_radii = radius(flat_dbf[fresh], scale, const, cap)
            out.voxels += [int(v) for v in fresh]
            out.radii += [int(r) for r in fresh_radii]
            out.before += [junction] + [int(v) for v in fresh[:-1]]
            out.offsets.append(len(out.voxels))
            out.branch_label.append(row)
            out.branch_round.append(rounds)
            out.branch_junction.append(junction)
            flat_skel[fresh] = True
            valid.reshape(-1)[fresh] = False      # r >= 0: a vertex is invalid even where a caller's box leaves it out
            n_live += 1
            n_new += len(fresh)
        out.live.append(n_live)
        out.new.append(n_new)
        out.states.append((valid * VALID + skeleton * SKELETON).astype(np.uint8))
    out.initial = eligible(labels, sources, hops, daf).astype(np.uint8)
    return out


def whole_paths(labels, sources, dbf, daf, parents, hops, scale, const, boxes=None, max_paths=None):
    """
    The kimimaro-shaped oracle, written on its own: it shares no walk, cube, target or radius code with
    incremental(). Every path goes to the root in plain Python, a full cube is stamped around every voxel of it
    through a Chebyshev distance on coordinate grids, the radius is Python float arithmetic (math.sqrt), and the
    round's new vertices are the path voxels that no earlier path held. Nothing clears a vertex but its own cube.
    """
    import math

    labels = np.ascontiguousarray(labels, dtype=np.int32)
    shape, k = labels.shape, len(sources) - 1
    flat_l = labels.reshape(-1)
    flat_daf = np.ascontiguousarray(daf, dtype=np.float32).reshape(-1)
    flat_dbf, flat_p, flat_h = (np.asarray(a).reshape(-1) for a in (dbf, parents, hops))
    zz, yy, xx = np.indices(shape)
    # the eligible voxels, row by row
    valid = np.zeros(labels.size, dtype=bool)
    for row in range(1, k + 1):
        s = int(sources[row])
        if 0 <= s < labels.size and flat_l[s] == row:
            for v in np.flatnonzero(flat_l == row):
                bits = int(flat_daf[v:v + 1].view(np.uint32)[0])
                valid[v] = flat_h[v] >= 0 and bits < 0x7F800000
    out = Result()
    out.initial = valid.reshape(shape).astype(np.uint8)
    on_skeleton = set()
    finished = set()
    rounds = 0
    while max_paths is None or rounds < max_paths:
        todo = []
        for row in range(1, k + 1):
            mine = [int(v) for v in np.flatnonzero(valid & (flat_l == row))]
            if mine and row not in finished:
                todo.append((row, min(mine, key=lambda v: (-int(flat_daf[v:v + 1].view(np.uint32)[0]), v))))
        if not todo:
            break
        rounds += 1
        n_live = n_new = 0
        for row, target in todo:
            path, v, broken = [target], target, False
            for _ in range(int(flat_h[target])):
                p = int(flat_p[v])
                if p < 0 or p >= labels.size or p == v:
                    broken = True
                    break
                path.append(p)
                v = p
            if broken or int(flat_p[v]) != v:
                out.broken += 1
                finished.add(row)
                continue
            path.reverse()      # root first
            if boxes is None:
                where = np.nonzero(labels == row)
                box = [int(w.min()) for w in where] + [int(w.max()) + 1 for w in where]
            else:
                box = [int(b) for b in boxes[row]]
            inside = ((labels == row) & (zz >= box[0]) & (zz < box[3]) & (yy >= box[1]) & (yy < box[4])
                      & (xx >= box[2]) & (xx < box[5]))
            radii = []
            for p in path:
                x = float(scale) * math.sqrt(float(max(int(flat_dbf[p]), 0))) + float(const)
                r = max(shape) if x >= max(shape) else math.floor(x)
                radii.append(r)
                pz, py, px = (int(c) for c in np.unravel_index(p, shape))
                near = np.maximum(np.maximum(np.abs(zz - pz), np.abs(yy - py)), np.abs(xx - px)) <= r
                valid &= ~(near & inside).reshape(-1)
            fresh = [i for i, p in enumerate(path) if p not in on_skeleton]
            junction = path[fresh[0] - 1] if fresh[0] > 0 else -1
            assert fresh == list(range(fresh[0], len(path)))      # the skeleton is closed under parents
            out.voxels += [path[i] for i in fresh]
            out.radii += [radii[i] for i in fresh]
            out.before += [junction] + [path[i] for i in fresh[:-1]]
            out.offsets.append(len(out.voxels))
            out.branch_label.append(row)
            out.branch_round.append(rounds)
            out.branch_junction.append(junction)
            on_skeleton.update(path)
            n_live += 1
            n_new += len(fresh)
        out.live.append(n_live)
        out.new.append(n_new)
        state = valid.astype(np.uint8) * VALID
        state[sorted(on_skeleton)] |= SKELETON
        out.states.append(state.reshape(shape))
    return out


def incremental(labels, sources, dbf, daf, parents, hops, scale, const, boxes=None, max_paths=None):
    """The device's form: junction stop, cube differences."""
    return _run(labels, sources, dbf, daf, parents, hops, scale, const, boxes, max_paths)


# ---- volumes -----------------------------------------------------------------------------------------
def dbf_of(labels):
    """distance_to_boundary's field from its own oracle (tests/dbf_ref.py: a per-label EDT, exact)."""
    import dbf_ref

    return dbf_ref.per_label(np.ascontiguousarray(labels, dtype=np.int32))


def fields_of(labels, sources, cost=None):
    """(daf, parents, hops) of the oracles of geodesic_field and geodesic_parents: the Euclidean field as the
    priority, the parental field of the cost field (of the Euclidean one without a cost)."""
    import parents_ref as pref

    daf = ref.relaxation(labels, sources)
    field = daf if cost is None else ref.relaxation(labels, sources, cost)
    parents, hops, orphans, _ = pref.jacobi(labels, sources, field, cost)
    assert orphans == 0
    return daf, parents, hops


def case(labels, sources, cost=None, dbf=None):
    """Every input of the loop for given labels and sources: (labels, sources, dbf, daf, parents, hops)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    sources = np.asarray(sources, dtype=np.int32)
    daf, parents, hops = fields_of(labels, sources, cost)
    if dbf is None:
        dbf = dbf_of(labels)
    return labels, sources, np.ascontiguousarray(dbf, dtype=np.int32), daf, parents, hops


def seeded(seed, **kw):
    """geodesic_ref.seeded_case(seed) with the loop's inputs; odd seeds walk the parents of a cost field."""
    labels, sources, cost = ref.seeded_case(seed, **kw)
    return case(labels, sources, cost)


def index_of(shape, v):
    return int(np.ravel_multi_index(v, shape))


def line(length, axis, at=0):
    """A one-voxel line of "length" along "axis" through a 3 x 3 cross-section, the source at position "at"."""
    shape = [3, 3, 3]
    shape[axis] = length
    labels = np.zeros(shape, dtype=np.int32)
    where = [1, 1, 1]
    where[axis] = slice(None)
    labels[tuple(where)] = 1
    where[axis] = at
    return case(labels, [-1, index_of(shape, where)])


def y_shape():
    """A stem along x that forks into two diagonal arms of unequal length at (1, 8, 10); the source at the stem's end."""
    shape = (3, 17, 24)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 8, :11] = 1
    for i in range(1, 8):
        labels[1, 8 - i, 10 + i] = 1
    for i in range(1, 6):
        labels[1, 8 + i, 10 + i] = 1
    return case(labels, [-1, index_of(shape, (1, 8, 0))])


def comb(teeth=5):
    """A spine along x with "teeth" teeth along y, the last at the spine's end; the source at the spine's start."""
    shape = (3, 9, 4 * teeth + 2)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 1, :4 * teeth + 1] = 1
    for t in range(1, teeth + 1):
        labels[1, 2:8, 4 * t] = 1
    return case(labels, [-1, index_of(shape, (1, 1, 0))])


def cross(arm=5):
    """A plus in the plane z = 1, the source in the centre, four arms of equal length: the tips' daf bits tie."""
    side = 2 * arm + 1
    shape = (3, side, side)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, arm, :] = 1
    labels[1, :, arm] = 1
    return case(labels, [-1, index_of(shape, (1, arm, arm))])


def wavy_block(shape=(14, 15, 36)):
    """A solid label that touches every face, with a field in place of the dbf that rises and falls along every
    path: the radii of neighbouring vertices differ by up to a few voxels in both directions."""
    labels = np.ones(shape, dtype=np.int32)
    z, y, x = np.indices(shape)
    wave = np.abs((x + 2 * y + z) % 10 - 5)
    return case(labels, [-1, 0], dbf=(wave * wave).astype(np.int32))


def slab_census(result, labels, dbf, scale, const, boxes=None):
    """
    Which of the six slabs of "cube minus the previous vertex's cube" are non-empty for some vertex of a
    result: a set out of "z-", "z+", "y-", "y+", "x-", "x+", plus "whole" for a cube without a previous one
    or apart from it, and "none" for a cube that lies inside the previous one.
    """
    shape, k = labels.shape, int(max(result.branch_label, default=0))
    boxes = boxes_of(labels, k) if boxes is None else boxes
    flat, cap, seen = np.asarray(dbf).reshape(-1), max(shape), set()
    rows = np.repeat(result.branch_label, np.diff(result.offsets))
    for v, prev, row in zip(result.voxels, result.before, rows):
        a = _cube(shape, boxes[row], v, radius(flat[v], scale, const, cap))
        b = None if prev < 0 else _cube(shape, boxes[row], prev, radius(flat[prev], scale, const, cap))
        if a is None:
            continue
        if b is None or any(max(p.start, q.start) >= min(p.stop, q.stop) for p, q in zip(a, b)):
            seen.add("whole")
            continue
        found = False
        for axis, name in enumerate("zyx"):
            if a[axis].start < b[axis].start:
                seen.add(name + "-")
                found = True
            if a[axis].stop > b[axis].stop:
                seen.add(name + "+")
                found = True
        if not found:
            seen.add("none")
    return seen
