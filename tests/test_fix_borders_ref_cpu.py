"""
tests/fix_borders_ref.py against the oracles it extends (no GPU): without given targets it reproduces
teasar_ref.incremental and fix_branching_ref.loop exactly, arrays and the state after every round; with the border
targets of tests/border_ref.py every eligible one is a skeleton vertex at the end, a label's result does not depend
on the other labels' targets, rounds without a branch are recorded, and max_paths counts them.
"""

import numpy as np
import pytest

import border_ref
import fix_borders_ref as fx
import fix_branching_ref as fb
import teasar_ref as tref

SCALE, CONST = 1.25, 1.0


def same(a, b):
    for x, y in zip(a.arrays(), b.arrays()):
        np.testing.assert_array_equal(x, y)
    assert a.before == b.before and a.live == b.live and a.new == b.new and len(a.states) == len(b.states)
    for x, y in zip(a.states, b.states):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.initial, b.initial)


@pytest.mark.parametrize("make", [tref.y_shape, tref.comb, tref.cross, lambda: tref.seeded(3), lambda: tref.seeded(4)])
def test_without_given_targets_it_is_teasar_ref(make):
    inputs = make()
    for max_paths in (None, 2):
        want = tref.incremental(*inputs, SCALE, CONST, max_paths=max_paths)
        got = fx.single(*inputs, SCALE, CONST, max_paths=max_paths)
        same(got, want)
        assert got.empty == [] and len(want.states) >= 2


@pytest.mark.parametrize("make", [lambda: fb.with_cost(tref.y_shape()), fb.touching, lambda: fb.seeded(3)])
def test_without_given_targets_it_is_fix_branching_ref(make):
    inputs = make()
    want = fb.loop(*inputs, SCALE, CONST)
    got = fx.loop(*inputs, SCALE, CONST)
    same(got, want)
    assert got.empty == []


def border_given(labels, k):
    rows = border_ref.brute_force(labels, k)
    return rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32)


@pytest.mark.parametrize("name", sorted(fx.CASES))
@pytest.mark.parametrize("form", ["single", "loop"])
def test_every_eligible_given_target_ends_on_the_skeleton(name, form):
    labels, sources, dbf, daf, cost = fx.CASES[name]()
    k = len(sources) - 1
    given = border_given(labels, k)
    assert len(given[0]) >= 2
    if form == "single":
        single = fb.single_field(labels, sources, dbf, daf, cost, SCALE, CONST)      # its parents, through the oracle
        import geodesic_ref as ref
        import parents_ref as pref
        field = ref.relaxation(labels, sources, cost)
        parents, hops, _, _ = pref.jacobi(labels, sources, field, cost)
        got = fx.single(labels, sources, dbf, daf, parents, hops, SCALE, CONST, given)
        plain = single
    else:
        got = fx.loop(labels, sources, dbf, daf, cost, SCALE, CONST, given)
        plain = fb.loop(labels, sources, dbf, daf, cost, SCALE, CONST)
    sets = got.vertex_sets(k)
    eligible = sum(len(v) for v in got.given.values())
    assert 1 <= eligible <= len(given[0])
    for row, voxels in got.given.items():
        assert set(voxels) <= sets[row], (row, voxels)
    final = got.states[-1]
    assert not (final & tref.VALID).any()      # the loop ran to its end
    assert len(got.states) >= max(len(v) for v in got.given.values())
    assert got.live[0] == plain.live[0]      # round 1: every rooted label has a branch, as without targets
    if name == "pieces":
        dropped = len(given[0]) - eligible
        assert dropped >= 1      # the far piece's targets are not eligible
    # a label alone, with its own targets only, gives the same branches
    for row in range(1, k + 1):
        keep = given[0] == row
        alone = (fx.single(labels, sources, dbf, daf, parents, hops, SCALE, CONST, (given[0][keep], given[1][keep]))
                 if form == "single" else None)
        if alone is not None:
            assert alone.vertex_sets(k)[row] == sets[row]


def test_rounds_without_a_branch_and_max_paths():
    """The comb's spine lies on the face y = 0 and its source at the spine's far end: the first given target, the
    spine's first voxel, puts the whole spine on the skeleton, so the rounds of the other spine voxels are empty.
    They are recorded and count for max_paths."""
    labels, sources, dbf, daf, cost = fx.faces_comb(source_at_end=True)
    spine = np.nonzero(labels.reshape(-1) == 1)[0]
    spine = spine[(spine // labels.shape[2]) % labels.shape[1] == 0]      # the voxels of the row y = 0
    given = (np.ones(len(spine), dtype=np.int32), spine.astype(np.int32)[::-1].copy())      # any order
    got = fx.loop(labels, sources, dbf, daf, cost, SCALE, 0.0, given)
    assert got.given[1] == sorted(spine.tolist())
    assert got.empty and got.empty[0] >= 2 and all(got.live[t - 1] == 0 for t in got.empty)
    assert len(got.states) >= len(spine)      # every given round is run
    for t in got.empty:
        np.testing.assert_array_equal(got.states[t - 1], got.states[t - 2])
    cut = fx.loop(labels, sources, dbf, daf, cost, SCALE, 0.0, given, max_paths=got.empty[0] + 1)
    assert len(cut.states) == got.empty[0] + 1
    for x, y in zip(cut.states, got.states):
        np.testing.assert_array_equal(x, y)
