"""
CPU oracles of the seeded fields (exaspim_geodesic_reseed, exaspim_geodesic_parents_begin_seeds) and of
teasar_branches_fix_branching, written from the definition, and the volumes the CPU and GPU tests
share.

The definition: labels, K, adjacency and the weights w(u -> v) are geodesic_ref.py's. seeds is a list of C-order
linear indices, any number per label, duplicates allowed; a seed is valid iff it lies in the volume and its label
is in 1..K. The seeded field d is the least solution of d[seed] = +0.0 at every valid seed and
d[v] = min over adjacent u of fl32(d[u] + w(u -> v)): a seed's own cost is never read, a label without a seed
stays +inf. Seeded hops and parents are parents_ref.py's with "the source" read as "a seed": h = 0 at every valid
seed whose field word is +0.0, no tight edge enters a seed, a seed is its own parent.

The loop: round 1 is teasar_ref's round 1. Before the walk of round t >= 2 the penalty field is the seeded field
of all the skeleton's vertices, and hops and parents are rebuilt with them as seeds; the target, the walk to the
first skeleton voxel and the invalidation are teasar_ref's.

  seeded_field    a multi-source float32 heap Dijkstra per label; with "start" the incremental form: the given
                  field, zeroed at the seeds, relaxed from them only.
  seeded_parents  a breadth-first search over tight edges from all seeds and the parent rule, in plain Python.
  loop            one serial loop per label, put together in the device's order. form="seeds" is oracle (A): a
                  Dijkstra from all skeleton voxels, from scratch, every round. form="incremental" zeroes the
                  round's new vertices in the field of the round before. form="zeroed" is oracle (B), kimimaro's
                  wording: the cost zeroed on the skeleton, the root as the only source.
"""

import heapq

import numpy as np

import geodesic_ref as ref
import teasar_ref as tref

INF = float("inf")


class Graph:
    """The 26-neighbourhood inside labels 1..K on flat indices, neighbours in ascending index order, cached."""

    def __init__(self, labels, k, cost=None):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32)
        self.shape, self.n, self.k = self.labels.shape, self.labels.size, int(k)
        flat = self.labels.reshape(-1)
        self.joined = np.where((flat >= 1) & (flat <= k), flat, 0).tolist()
        self.weights = None if cost is None else weights_of(cost)
        self._cache = {}

    def neighbours(self, u):
        """[(v, the Euclidean step u <-> v as a float)], v ascending."""
        out = self._cache.get(u)
        if out is None:
            d, h, w = self.shape
            z, y, x = u // (h * w), (u // w) % h, u % w
            me, out = self.joined[u], []
            for dz, dy, dx in ref.OFFSETS:
                a, b, c = z + dz, y + dy, x + dx
                if 0 <= a < d and 0 <= b < h and 0 <= c < w:
                    v = (a * h + b) * w + c
                    if self.joined[v] == me:
                        out.append((v, float(ref.STEP[(dz != 0) + (dy != 0) + (dx != 0)])))
            self._cache[u] = out
        return out

    def valid_seeds(self, seeds):
        """(the valid seeds, the number of invalid rows)."""
        good = [int(s) for s in seeds if 0 <= int(s) < self.n and self.joined[int(s)]]
        return good, len(seeds) - len(good)


def weights_of(cost):
    """The entering weights of a cost volume as a flat list of floats (each a float32 value or inf)."""
    return ref.entering_weight(cost).reshape(-1).astype(np.float64).tolist()


def _fl32(x):
    """A double rounded to float32. The double sum of two float32 is then the one rounded float32 addition
    (53 >= 2 * 24 + 2 bits: rounding twice is harmless)."""
    return float(np.float32(x))


def seeded_field(graph, seeds, weights="graph", start=None):
    """
    float32 (D, H, W): the seeded field, by a heap Dijkstra in float32. "weights" overrides the graph's entering
    weights (a flat list, or None for Euclidean steps). "start" is a converged field of other seeds: it is zeroed
    at "seeds" and relaxed from them only (the incremental form).
    """
    weights = graph.weights if isinstance(weights, str) else weights
    seeds, _ = graph.valid_seeds(seeds)
    if start is None:
        d = np.where(graph.labels.reshape(-1) > 0, np.float32(np.inf), np.float32(0)).astype(np.float64).tolist()
    else:
        d = np.ascontiguousarray(start, dtype=np.float32).reshape(-1).astype(np.float64).tolist()
    heap = []
    for s in set(seeds):
        d[s] = 0.0
        heap.append((0.0, s))
    heapq.heapify(heap)
    while heap:
        du, u = heapq.heappop(heap)
        if du > d[u]:
            continue
        for v, step in graph.neighbours(u):
            w = step if weights is None else weights[v]
            if w == INF:
                continue
            dv = _fl32(du + w)
            if dv < d[v]:
                d[v] = dv
                heapq.heappush(heap, (dv, v))
    return np.array(d, dtype=np.float64).astype(np.float32).reshape(graph.shape)


def seeded_parents(graph, seeds, field, weights="graph"):
    """(parents int32, hops int32, orphans, invalid rows) of a seeded field: breadth first over tight edges."""
    weights = graph.weights if isinstance(weights, str) else weights
    words = ref.bits(np.ascontiguousarray(field, dtype=np.float32)).reshape(-1)
    d = np.asarray(field, dtype=np.float32).reshape(-1).astype(np.float64).tolist()
    good, invalid = graph.valid_seeds(seeds)
    invalid += sum(1 for s in good if words[s] != 0)
    good = sorted({s for s in good if words[s] == 0})
    is_seed = set(good)
    hops = np.full(graph.n, -1, dtype=np.int32)
    parents = np.full(graph.n, -1, dtype=np.int32)

    def tight(u, v, step):      # u -> v, adjacent and of one label
        if v in is_seed or d[u] == INF or d[v] == INF:
            return False
        w = step if weights is None else weights[v]
        return w != INF and _fl32(d[u] + w) == d[v]

    for s in good:
        hops[s] = 0
        parents[s] = s
    queue, at = list(good), 0
    while at < len(queue):
        u = queue[at]
        at += 1
        for v, step in graph.neighbours(u):
            if hops[v] < 0 and tight(u, v, step):
                hops[v] = hops[u] + 1
                queue.append(v)
    orphans = 0
    for v in range(graph.n):
        if not graph.joined[v] or d[v] == INF or v in is_seed:
            continue
        before = [u for u, step in graph.neighbours(v) if tight(u, v, step)]
        if not before:
            orphans += 1
        for u in before:      # ascending: the first is the smallest index
            if hops[v] >= 1 and hops[u] == hops[v] - 1:
                parents[v] = u
                break
    return parents.reshape(graph.shape), hops.reshape(graph.shape), orphans, invalid


def chain_adds_up(graph, parents, field, target, weights="graph"):
    """Whether re-adding the weights along the parents from the seed to "target" gives the field at every voxel."""
    weights = graph.weights if isinstance(weights, str) else weights
    flat_p = parents.reshape(-1)
    d = np.asarray(field, dtype=np.float32).reshape(-1)
    chain = [int(target)]
    while flat_p[chain[-1]] != chain[-1]:
        chain.append(int(flat_p[chain[-1]]))
        if chain[-1] < 0 or len(chain) > graph.n:
            return False
    chain.reverse()
    total = np.float32(0)
    if ref.bits(d[chain[0]:chain[0] + 1])[0] != 0:
        return False
    for u, v in zip(chain, chain[1:]):
        step = dict(graph.neighbours(u)).get(v)
        if step is None:
            return False
        total = np.float32(total + np.float32(step if weights is None else weights[v]))
        if ref.bits(np.array([total]))[0] != ref.bits(d[v:v + 1])[0]:
            return False
    return True


def loop(labels, sources, dbf, daf, cost, scale, const, boxes=None, max_paths=None, form="seeds"):
    """
    The fix_branching loop, one label after the other, as a teasar_ref.Result in the device's order, with
    .fields[(label, round)] the float32 field of the label's voxels that round's walk used, .label_voxels[label]
    their indices, and .chains the number of branches whose chain was re-added to the field (all of them must).
    """
    assert form in ("seeds", "incremental", "zeroed")
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    shape, k = labels.shape, len(sources) - 1
    graph = Graph(labels, k, cost)
    assert form != "zeroed" or graph.weights is not None
    if boxes is None:
        boxes = tref.boxes_of(labels, k)
    cap = max(shape)
    flat_l, flat_dbf = labels.reshape(-1), np.asarray(dbf).reshape(-1)
    words = ref.bits(np.ascontiguousarray(daf, dtype=np.float32)).view(np.uint32).reshape(-1)
    good, _ = ref.valid_sources(labels, sources)
    per_label = {}      # label -> [(vertices ascending hops, radii, junction, the label's state bytes after the round)]
    fields, label_voxels, chains = {}, {}, 0
    initial = np.zeros(labels.size, dtype=np.uint8)
    for row in range(1, k + 1):
        if good[row] < 0:
            continue
        root = int(good[row])
        mine = np.nonzero(flat_l == row)[0]
        label_voxels[row] = mine
        field = seeded_field(graph, [root])
        valid = np.zeros(labels.size, dtype=bool)
        valid[mine] = np.isfinite(field.reshape(-1)[mine]) & (words[mine] < 0x7F800000)
        initial[valid] = tref.VALID
        skeleton = np.zeros(labels.size, dtype=bool)
        vertices, fresh, rounds = [], [], []
        zeroed = None if graph.weights is None else list(graph.weights)
        while valid.any() and (max_paths is None or len(rounds) < max_paths):
            if rounds:
                if form == "seeds":
                    field = seeded_field(graph, vertices)
                elif form == "incremental":
                    field = seeded_field(graph, fresh, start=field)
                else:
                    for v in fresh:
                        zeroed[v] = 0.0
                    field = seeded_field(graph, [root], weights=zeroed)
            seeds = vertices if rounds else [root]
            # the parents of the zeroed form are not the seeded ones: its walk is taken on the seeded definition
            parents, hops, orphans, invalid = seeded_parents(graph, seeds, field)
            assert orphans == 0 and invalid == 0, (row, len(rounds) + 1, orphans, invalid)
            fields[(row, len(rounds) + 1)] = field.reshape(-1)[mine].copy()
            where = np.nonzero(valid)[0]
            top = words[where].max()
            target = int(where[words[where] == top].min())
            walked = tref._walk(parents.reshape(-1), hops.reshape(-1), skeleton, target, labels.size)
            assert walked is not None
            path, junction = walked
            assert len(path) == int(hops.reshape(-1)[target]) + (junction < 0)      # the junction is the self-parent
            chains += chain_adds_up(graph, parents, field, target)
            fresh = path[::-1]
            radii = tref.radius(flat_dbf[fresh], scale, const, cap)
            own = (labels == row)
            state = valid.reshape(shape)
            for v, r in zip(fresh, radii):      # whole cubes: the cube of the vertex before was cleared before
                cube = tref._cube(shape, boxes[row], v, r)
                if cube is not None:
                    state[cube] &= ~own[cube]
            valid[fresh] = False
            skeleton[fresh] = True
            vertices = vertices + fresh
            rounds.append((fresh, [int(r) for r in radii], junction,
                           (valid[mine] * tref.VALID + skeleton[mine] * tref.SKELETON).astype(np.uint8)))
        per_label[row] = rounds
    out = tref.Result()
    out.initial = initial.reshape(shape)
    out.fields, out.label_voxels, out.chains = fields, label_voxels, chains
    t = 0
    while any(len(r) > t for r in per_label.values()):
        state = np.zeros(labels.size, dtype=np.uint8) if t == 0 else out.states[-1].reshape(-1).copy()
        if t == 0:
            state[:] = initial
        n_live = n_new = 0
        for row in sorted(per_label):
            if len(per_label[row]) <= t:
                continue
            fresh, radii, junction, bytes_ = per_label[row][t]
            state[label_voxels[row]] = bytes_
            out.voxels += fresh
            out.radii += radii
            out.before += [junction] + fresh[:-1]
            out.offsets.append(len(out.voxels))
            out.branch_label.append(row)
            out.branch_round.append(t + 1)
            out.branch_junction.append(junction)
            n_live += 1
            n_new += len(fresh)
        out.live.append(n_live)
        out.new.append(n_new)
        out.states.append(state.reshape(shape))
        t += 1
    return out


# ---- volumes -----------------------------------------------------------------------------------------
def penalty(labels, sources, dbf, daf):
    """A TEASAR-shaped penalty without the device's chain: large away from the label's core, plus the daf."""
    dbf = np.asarray(dbf, dtype=np.float32)
    peak = max(float(np.sqrt(dbf.max())), 1.0)
    finite = np.where(np.isfinite(daf), daf, 0).astype(np.float32)
    far = max(float(finite.max()), 1.0)
    cost = (np.float32(1000.0) * (1 - np.sqrt(dbf) / np.float32(peak)) ** 4 + finite / np.float32(far)).astype(np.float32)
    return np.where(np.asarray(labels) > 0, cost, np.float32(0)).astype(np.float32)


def seeded(seed):
    """teasar_ref.seeded(seed) with a cost for every seed: (labels, sources, dbf, daf, cost). Odd seeds keep
    geodesic_ref's random cost with its special values, even seeds get one drawn here."""
    labels, sources, cost = ref.seeded_case(seed)
    labels, sources, dbf, daf, _, _ = tref.seeded(seed)
    if cost is None:
        cost = ref.random_cost(np.random.default_rng(5000 + seed), labels.shape)
    return labels, sources, dbf, daf, cost


def thick_t():
    """
    The crafted volume where the two forms differ: a thick bar along x, the source at one end, and a thick stem
    that leaves the bar's far side. With one parental field the stem's path runs beside the first path towards
    the root; re-seeded, it joins the first path where that is cheapest. (labels, sources, dbf, daf, cost).
    """
    shape = (5, 20, 40)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1:4, 2:7, 1:39] = 1
    labels[1:4, 7:19, 24:29] = 1
    sources = np.array([-1, tref.index_of(shape, (2, 4, 1))], dtype=np.int32)
    labels, sources, dbf, daf, _, _ = tref.case(labels, sources)
    return labels, sources, dbf, daf, penalty(labels, sources, dbf, daf)


def with_cost(inputs):
    """A teasar_ref case (labels, sources, dbf, daf, parents, hops) as (labels, sources, dbf, daf, cost)."""
    labels, sources, dbf, daf, _, _ = inputs
    return labels, sources, dbf, daf, penalty(labels, sources, dbf, daf)


def from_labels(labels, sources=None):
    """(labels, sources, dbf, daf, cost) of a label volume: each label's first voxel as its source unless given."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    k = max(int(labels.max()), 1)
    if sources is None:
        sources = ref.first_voxels(labels, k)
    return with_cost(tref.case(labels, sources))


def touching():
    """Two thick L-shaped labels that touch along a plane, in a volume that crosses a tile seam on every axis."""
    labels = np.zeros((9, 17, 40), dtype=np.int32)
    labels[1:8, 1:6, 1:39] = 1
    labels[1:8, 6:16, 1:6] = 1
    labels[1:8, 6:11, 6:39] = 2      # touches label 1 along y = 6 and along x = 6
    labels[1:8, 11:16, 30:39] = 2
    return from_labels(labels)


def tile_seams(shape, k=5, fill=0.9, seed=0):
    """
    Labels 1..k in slabs along x over a whole volume with voxels knocked out, a block of label k + 2 (above K) and
    one of negative labels: (labels, k). Every tile seam of the 8 x 8 x 32 tiles runs through foreground.
    """
    rng = np.random.default_rng(4000 + seed)
    x = np.indices(shape)[2]
    labels = (x * k // shape[2] + 1).astype(np.int32)
    labels[rng.random(shape) > fill] = 0
    labels[0:2, 0:3, 0:4] = k + 2
    labels[-2:, -3:, 0:4] = -3
    return labels, k


def seam_seeds(labels, k, without):
    """
    Seeds on the corners, edges and faces of the tiles and in the last partial tile of a tile_seams volume, made
    foreground where they were knocked out; label "without" gets none. Returns (labels, seeds as a list, some twice).
    """
    labels = labels.copy()
    d, h, w = labels.shape
    spots = [(7, 7, 31), (8, 8, 32), (7, 8, 31), (8, 7, 32),      # the corners where eight tiles meet
             (7, 3, 31), (3, 8, 32), (8, 7, 12),                  # edges
             (3, 3, 32), (4, 7, 10), (8, 12, 20),                 # faces
             (d - 1, h - 1, w - 1), (d - 1, 0, w - 2), (0, h - 1, 33), (0, 0, 5), (2, 2, 2)]
    spots = [s for s in spots if all(c < n for c, n in zip(s, labels.shape))]
    seeds = []
    for s in spots:
        row = int(s[2] * k // w + 1)
        if row == without:
            continue
        if (s[0] < 2 and s[1] < 3 and s[2] < 4) or (s[0] >= d - 2 and s[1] >= h - 3 and s[2] < 4):
            continue      # the blocks of labels outside 1..K
        labels[s] = row
        seeds.append(int(np.ravel_multi_index(s, labels.shape)))
    return labels, seeds + seeds[::3]


def absorbing(seed, shape=(9, 17, 40)):
    """
    geodesic_ref.seeded_case of an odd seed on a shape that crosses tile seams, its cost (zeros, -0.0, +inf, NaN,
    negatives) scaled by 3e7 with 1e-3 entries mixed in, so that small costs are absorbed next to large ones.
    """
    labels, sources, cost = ref.seeded_case(2 * seed + 1, shape=shape)
    rng = np.random.default_rng(7000 + seed)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (cost * np.float32(3e7)).astype(np.float32)
    cost = np.where(rng.random(cost.shape) < 0.3, np.float32(1e-3), scaled).astype(np.float32)
    return np.ascontiguousarray(labels, dtype=np.int32), len(sources) - 1, cost


def random_seeds(rng, labels, k, per_label):
    """Up to "per_label" random voxels of every label in 1..k, as a list."""
    flat = np.asarray(labels).reshape(-1)
    out = []
    for row in range(1, k + 1):
        where = np.nonzero(flat == row)[0]
        if where.size:
            out += [int(v) for v in rng.choice(where, size=min(per_label, where.size), replace=False)]
    return out


def single_field(labels, sources, dbf, daf, cost, scale, const, **kw):
    """teasar_ref.incremental on the parental field of the cost field: the fix_branching=False form."""
    import parents_ref as pref

    field = ref.relaxation(labels, sources, cost)
    parents, hops, orphans, _ = pref.jacobi(labels, sources, field, cost)
    assert orphans == 0
    return tref.incremental(labels, sources, dbf, daf, parents, hops, scale, const, **kw)
