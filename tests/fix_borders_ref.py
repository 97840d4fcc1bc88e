"""
CPU oracles of TEASAR's loops with given targets (exaspim_teasar_round_given, teasar_branches_given and
teasar_branches_fix_branching_given), written from the definition on the helpers of tests/teasar_ref.py
and tests/fix_branching_ref.py, and the volumes the CPU and GPU tests share.

The definition, per label, so that no label depends on another: the given targets of a label are the rows of
(target_labels, target_voxels) whose voxel is eligible before round 1, ascending, each once. In round t a label
with at least t of them takes the t-th as its target, whether it is still valid or not; if it is on the skeleton
already the label has no branch in that round. A label that has run out takes its valid voxel with the largest
daf bits, ties to the smallest index, and has no branch once it has none. The walk and the invalidation are
teasar_ref's. The rounds run until every label has run out of given targets and none has a valid voxel;
max_paths counts rounds, empty ones included.

  single   one parental field for every round (teasar_ref.incremental's form).
  loop     the parental field rebuilt from the whole skeleton before every round after the first
           (fix_branching_ref.loop's form="seeds").

One label after the other, then re-ordered into the device's rounds as fix_branching_ref.loop does. Both return
a teasar_ref.Result whose .states has one entry per round, empty rounds included, with .empty the list of those.
"""

import numpy as np

import fix_branching_ref as fb
import geodesic_ref as ref
import teasar_ref as tref


def given_of(labels, initial, given, k):
    """label -> its eligible given voxels, ascending, each once. "initial" is the state before round 1."""
    out = {row: [] for row in range(1, k + 1)}
    if given is None:
        return out
    flat_l, flat_i = np.asarray(labels).reshape(-1), np.asarray(initial).reshape(-1)
    for row, v in zip(*given):
        row, v = int(row), int(v)
        assert 1 <= row <= k and 0 <= v < flat_l.size and flat_l[v] == row, (row, v)
        if flat_i[v] & tref.VALID:
            out[row].append(v)
    return {row: sorted(set(vs)) for row, vs in out.items()}


def _one_label(row, labels, valid, words, flat_dbf, box, scale, const, targets, fields, max_paths):
    """
    The serial loop of one label: a list with one entry per round, None for a round without a branch, else
    (vertices in ascending hops, radii, junction), and the state bytes of the label's voxels after every round.
    "valid" (flat, bool) is updated in place.
    """
    shape, n = labels.shape, labels.size
    own = labels == row
    skeleton = np.zeros(n, dtype=bool)
    vertices, rounds, bytes_ = [], [], []
    mine = np.nonzero(labels.reshape(-1) == row)[0]
    cap = max(shape)
    while max_paths is None or len(rounds) < max_paths:
        t = len(rounds) + 1
        if t <= len(targets):
            target = targets[t - 1]
            if skeleton[target]:
                target = None
        else:
            where = mine[valid[mine]]
            if not where.size:
                break
            top = words[where].max()
            target = int(where[words[where] == top].min())
        if target is None:
            rounds.append(None)
        else:
            parents, hops = fields(row, vertices)
            walked = tref._walk(parents, hops, skeleton, target, n)
            assert walked is not None, (row, t, target)
            path, junction = walked
            assert path and (junction >= 0) == bool(vertices)
            fresh = path[::-1]
            radii = tref.radius(flat_dbf[fresh], scale, const, cap)
            state = valid.reshape(shape)
            for v, r in zip(fresh, radii):      # whole cubes: the cube of the vertex before was cleared before
                cube = tref._cube(shape, box, v, r)
                if cube is not None:
                    state[cube] &= ~own[cube]
            valid[fresh] = False
            skeleton[fresh] = True
            vertices = vertices + fresh
            rounds.append((fresh, [int(r) for r in radii], junction))
        bytes_.append((valid[mine] * tref.VALID + skeleton[mine] * tref.SKELETON).astype(np.uint8))
    return mine, rounds, bytes_


def _assemble(labels, k, initial, per_label, given_rounds, max_paths):
    out = tref.Result()
    out.initial = initial.reshape(labels.shape).copy()
    out.empty = []
    total = max([given_rounds] + [len(r[1]) for r in per_label.values()])
    if max_paths is not None:
        total = min(total, max_paths)
    state = initial.reshape(-1).copy()
    for t in range(total):
        n_live = n_new = 0
        for row in sorted(per_label):
            mine, rounds, bytes_ = per_label[row]
            if len(rounds) <= t:
                continue
            state[mine] = bytes_[t]
            if rounds[t] is None:
                continue
            fresh, radii, junction = rounds[t]
            out.voxels += fresh
            out.radii += radii
            out.before += [junction] + fresh[:-1]
            out.offsets.append(len(out.voxels))
            out.branch_label.append(row)
            out.branch_round.append(t + 1)
            out.branch_junction.append(junction)
            n_live += 1
            n_new += len(fresh)
        if n_live == 0:
            out.empty.append(t + 1)
        out.live.append(n_live)
        out.new.append(n_new)
        out.states.append(state.reshape(labels.shape).copy())
    return out


def _run(labels, sources, dbf, daf, hops0, scale, const, given, boxes, max_paths, fields):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    k = len(sources) - 1
    if boxes is None:
        boxes = tref.boxes_of(labels, k)
    words = ref.bits(np.ascontiguousarray(daf, dtype=np.float32)).view(np.uint32).reshape(-1)
    initial = tref.eligible(labels, sources, hops0, daf).astype(np.uint8)
    valid = initial.reshape(-1).astype(bool)
    targets = given_of(labels, initial, given, k)
    good, _ = ref.valid_sources(labels, sources)
    flat_dbf = np.asarray(dbf).reshape(-1)
    per_label = {}
    for row in range(1, k + 1):
        if good[row] < 0:
            continue
        per_label[row] = _one_label(row, labels, valid, words, flat_dbf, boxes[row], scale, const, targets[row],
                                    fields, max_paths)
    given_rounds = max([0] + [len(v) for v in targets.values()])
    out = _assemble(labels, k, initial, per_label, given_rounds, max_paths)
    out.given = targets
    return out


def single(labels, sources, dbf, daf, parents, hops, scale, const, given=None, boxes=None, max_paths=None):
    """teasar_ref.incremental with given targets: one parental field."""
    flat_p, flat_h = np.asarray(parents).reshape(-1), np.asarray(hops).reshape(-1)
    return _run(labels, sources, dbf, daf, hops, scale, const, given, boxes, max_paths,
                lambda row, vertices: (flat_p, flat_h))


def loop(labels, sources, dbf, daf, cost, scale, const, given=None, boxes=None, max_paths=None):
    """fix_branching_ref.loop (form="seeds") with given targets: the fields rebuilt from the whole skeleton."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    k = len(sources) - 1
    graph = fb.Graph(labels, k, cost)
    good, _ = ref.valid_sources(labels, sources)
    cache = {}

    def fields(row, vertices):
        key = (row, len(vertices))
        if key not in cache:
            cache.clear()
            seeds = vertices if vertices else [int(good[row])]
            field = fb.seeded_field(graph, seeds)
            parents, hops, orphans, invalid = fb.seeded_parents(graph, seeds, field)
            assert orphans == 0 and invalid == 0
            cache[key] = (parents.reshape(-1), hops.reshape(-1))
        return cache[key]

    # eligibility: finite in the field of the roots, which is where hops >= 0
    roots = [int(s) for s in good[1:] if s >= 0]
    field0 = fb.seeded_field(graph, roots)
    hops0 = np.where(np.isfinite(field0) & (labels > 0), 0, -1)
    return _run(labels, sources, dbf, daf, hops0, scale, const, given, boxes, max_paths, fields)


# ---- volumes whose arms end on faces --------------------------------------------------------------------
def faces_y():
    """teasar_ref.y_shape's Y in a volume cut to its extent: the stem starts on x = 0 and both arms end on faces."""
    shape = (1, 14, 18)
    labels = np.zeros(shape, dtype=np.int32)
    labels[0, 8, :11] = 1
    for i in range(1, 8):
        labels[0, 8 - i, 10 + i] = 1      # ends at (0, 1, 17): the face x = W - 1
    for i in range(1, 6):
        labels[0, 8 + i, 10 + i] = 1      # ends at (0, 13, 15): the face y = H - 1
    return fb.with_cost(tref.case(labels, [-1, tref.index_of(shape, (0, 8, 0))]))


def faces_comb(teeth=4, source_at_end=False):
    """teasar_ref.comb with the teeth running into the face y = H - 1 and the spine on the face y = 0; the source
    at the spine's start or, with source_at_end, at its far end."""
    shape = (3, 7, 4 * teeth + 2)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 0, :4 * teeth + 1] = 1
    for t in range(1, teeth + 1):
        labels[1, 1:7, 4 * t] = 1
    return fb.with_cost(tref.case(labels, [-1, tref.index_of(shape, (1, 0, 4 * teeth if source_at_end else 0))]))


def faces_touching():
    """fix_branching_ref.touching without its margin of background: both labels are cut by several faces."""
    labels = np.zeros((5, 15, 24), dtype=np.int32)
    labels[:, 0:5, :] = 1
    labels[:, 5:15, 0:5] = 1
    labels[:, 5:10, 5:24] = 2
    labels[:, 10:15, 17:24] = 2
    return fb.from_labels(labels)


def faces_pieces():
    """A label in two 26-disconnected pieces, both on faces (the far piece's targets are dropped), two one-voxel
    labels in a corner and on a face, and a label that touches no face."""
    labels = np.zeros((4, 9, 16), dtype=np.int32)
    labels[0:2, 0:3, 0:6] = 1
    labels[2:4, 6:9, 10:16] = 1
    labels[0, 8, 0] = 2
    labels[3, 0, 8] = 3
    labels[1:3, 3:6, 7:9] = 4
    return fb.from_labels(labels)


def faces_thick_t():
    """fix_branching_ref.thick_t with the bar's far end and the stem's end on faces."""
    shape = (5, 18, 30)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1:4, 2:7, 1:30] = 1
    labels[1:4, 7:18, 18:23] = 1
    sources = np.array([-1, tref.index_of(shape, (2, 4, 1))], dtype=np.int32)
    labels, sources, dbf, daf, _, _ = tref.case(labels, sources)
    return labels, sources, dbf, daf, fb.penalty(labels, sources, dbf, daf)


CASES = {"y": faces_y, "comb": faces_comb, "touching": faces_touching, "pieces": faces_pieces, "thick_t": faces_thick_t}
