"""
The two oracles of tests/teasar_ref.py held to each other, without a GPU: tracing every path to the root and
stamping a whole cube around every voxel of it gives, after every round, the same valid voxels and the same
skeleton as stopping at the junction and clearing each new vertex's cube minus the cube of the vertex before
it. Then what a skeleton is: a tree that contains the root, with every eligible voxel within r of a vertex of
its label, every junction on a branch of an earlier round, and nothing valid left unless max_paths cut the loop.
"""

import numpy as np
import pytest

import geodesic_ref as ref
import holes_ref
import teasar_ref as tref

PARAMS = [(0.0, 0.0), (1.25, 0.0), (1.25, 2.0), (0.5, 1.0), (4.0, 0.5), (0.0, 3.0), (1.25, 450.0), (1.0 / 3.0, 0.1)]
_CASES = {}


def seeded(seed):
    """(inputs, scale, const) of one seed: shared, and left unchanged."""
    if seed not in _CASES:
        inputs = tref.seeded(seed)
        for a in inputs:
            a.setflags(write=False)
        _CASES[seed] = inputs
    return _CASES[seed], PARAMS[seed % len(PARAMS)]


def holes_case(seed):
    """holes_ref's labels (several touching blocks, punched), first voxels as sources."""
    if ("h", seed) not in _CASES:
        labels = holes_ref.seeded_volume(seed)
        labels = np.ascontiguousarray(labels[:10, :10, :12], dtype=np.int32)
        k = max(int(labels.max()), 1)
        inputs = tref.case(labels, ref.first_voxels(labels, k))
        for a in inputs:
            a.setflags(write=False)
        _CASES[("h", seed)] = inputs
    return _CASES[("h", seed)], PARAMS[(seed + 3) % len(PARAMS)]


CASES = [("seeded", s) for s in range(32)] + [("holes", s) for s in range(8)]


def get(kind, seed):
    return seeded(seed) if kind == "seeded" else holes_case(seed)


@pytest.mark.parametrize("kind,seed", CASES)
def test_both_forms_give_equal_masks_after_every_round_and_equal_vertices(kind, seed):
    inputs, (scale, const) = get(kind, seed)
    whole = tref.whole_paths(*inputs, scale, const)
    inc = tref.incremental(*inputs, scale, const)
    assert whole.broken == 0 and inc.broken == 0
    assert len(whole.states) == len(inc.states)
    for t, (a, b) in enumerate(zip(whole.states, inc.states)):
        np.testing.assert_array_equal(a, b, err_msg=f"round {t + 1}")
    for a, b in zip(whole.arrays(), inc.arrays()):
        np.testing.assert_array_equal(a, b)
    assert whole.before == inc.before and whole.live == inc.live and whole.new == inc.new


@pytest.mark.parametrize("kind,seed", CASES)
def test_what_a_skeleton_is(kind, seed):
    inputs, (scale, const) = get(kind, seed)
    labels, sources, dbf, daf, parents, hops = inputs
    k = len(sources) - 1
    out = tref.incremental(*inputs, scale, const)
    voxels, radii, offsets, branch_label, branch_round, branch_junction = out.arrays()
    flat_l, flat_p, flat_h = labels.reshape(-1), parents.reshape(-1), hops.reshape(-1)
    start = tref.eligible(labels, sources, hops, daf)
    good, _ = ref.valid_sources(labels, sources)
    # nothing valid is left, and the skeleton bits are the vertices
    final = out.states[-1] if out.states else start.astype(np.uint8)
    assert not (final & tref.VALID).any()
    assert sorted(np.nonzero(final.reshape(-1) & tref.SKELETON)[0].tolist()) == sorted(voxels.tolist())
    assert len(set(voxels.tolist())) == len(voxels)
    sets = out.vertex_sets(k)
    for row in range(1, k + 1):
        mine = sets[row]
        if not (start & (labels == row)).any():
            assert not mine
            continue
        # a tree that contains the root: every vertex but the root has its parent on the skeleton
        assert int(good[row]) in mine
        for v in mine:
            assert flat_l[v] == row
            assert int(flat_p[v]) in mine      # the root is its own parent
        # every eligible voxel lies within r of a vertex of its label, inside the label's box by construction
        vs = np.array(sorted(mine))
        rs = tref.radius(dbf.reshape(-1)[vs], scale, const, max(labels.shape))
        coords = np.stack(np.unravel_index(vs, labels.shape), axis=1)
        for q in zip(*np.nonzero(start & (labels == row))):
            assert (np.abs(coords - np.array(q)).max(axis=1) <= rs).any(), (row, q)
    # every junction lies on a branch of an earlier round of the same label; round 1 has none
    seen = {}
    for b in range(len(branch_label)):
        row, t, j = int(branch_label[b]), int(branch_round[b]), int(branch_junction[b])
        branch = voxels[offsets[b]:offsets[b + 1]]
        np.testing.assert_array_equal(np.diff(flat_h[branch]), 1)      # ascending hops, junction side first
        if j < 0:
            assert t == min(branch_round[branch_label == row]) and flat_h[branch[0]] == 0
        else:
            assert j in seen[row] and flat_p[branch[0]] == j
        seen.setdefault(row, set()).update(branch.tolist())
    # the order: rounds, then labels ascending
    keys = list(zip(branch_round.tolist(), branch_label.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    np.testing.assert_array_equal(radii, tref.radius(dbf.reshape(-1)[voxels], scale, const, max(labels.shape)))


@pytest.mark.parametrize("seed", [2, 9, 12])
@pytest.mark.parametrize("max_paths", [1, 2])
def test_max_paths_cuts_the_loop_and_is_a_prefix(seed, max_paths):
    inputs, _ = seeded(seed)
    full = tref.incremental(*inputs, 0.0, 0.0)
    cut = tref.incremental(*inputs, 0.0, 0.0, max_paths=max_paths)
    whole = tref.whole_paths(*inputs, 0.0, 0.0, max_paths=max_paths)
    assert len(full.states) > max_paths      # one voxel per vertex: many rounds
    assert len(cut.states) == max_paths
    for a, b, c in zip(cut.states, full.states, whole.states):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert (cut.states[-1] & tref.VALID).any()
    n = cut.offsets[-1]
    assert cut.voxels == full.voxels[:n] and cut.radii == full.radii[:n]


def test_the_radius_formula_is_numpys():
    d2 = np.array([-5, 0, 1, 2, 3, 4, 15, 16, 17, 2**31 - 2, tref.DBF_INF], dtype=np.int32)
    np.testing.assert_array_equal(tref.radius(d2, 1.25, 0.0, 10**6), [0, 0, 1, 1, 2, 2, 4, 5, 5, 57926, 57926])
    np.testing.assert_array_equal(tref.radius(d2, 1.25, 450.0, 100), [100] * len(d2))
    np.testing.assert_array_equal(tref.radius(d2, 0.0, 0.0, 100), [0] * len(d2))
    np.testing.assert_array_equal(tref.radius(d2, 1e308, 1e308, 7), [7] * len(d2))
    assert tref.radius(d2, 1.25, 2.0, 10**6).dtype == np.int64


def test_a_broken_walk_is_counted_and_finishes_its_label():
    inputs, _ = seeded(9)
    labels, sources, dbf, daf, parents, hops = inputs
    target = int(np.argmax(np.where(tref.eligible(labels, sources, hops, daf), daf, -1).reshape(-1)))
    chain = [target]
    while parents.reshape(-1)[chain[-1]] != chain[-1]:
        chain.append(int(parents.reshape(-1)[chain[-1]]))
    assert len(chain) >= 4
    row = int(labels.reshape(-1)[target])
    for poison in (-1, labels.size, 2**31 - 1, chain[2]):
        spoiled = parents.copy()
        spoiled.reshape(-1)[chain[2]] = poison
        out = tref.incremental(labels, sources, dbf, daf, spoiled, hops, 1.25, 0.0)
        assert out.broken == 1 and row not in out.branch_label
        assert (out.states[-1][labels == row] == out.initial[labels == row]).all() if out.states else True
