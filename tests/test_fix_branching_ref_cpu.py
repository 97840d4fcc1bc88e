"""
The oracles of tests/fix_branching_ref.py held to each other, without a GPU: the field seeded from the whole
skeleton (A) equals, bit for bit and after every round, the field of the cost zeroed along the skeleton with the
root as the only source (B, kimimaro's wording) and the field of the round before re-seeded with the round's new
vertices (the incremental form); every branch's chain of parents re-adds to the field; on a crafted volume the
loop gives other vertices than the single-parental-field loop of tests/teasar_ref.py, and where every label has
one path the two are equal.
"""

import numpy as np
import pytest

import fix_branching_ref as fb
import geodesic_ref as ref
import parents_ref as pref
import teasar_ref as tref
from test_teasar_ref_cpu import PARAMS

SEEDS = list(range(40))
_CASES, _RUNS = {}, {}


def case(seed):
    """(inputs, scale, const) of one seed: shared, and left unchanged."""
    if seed not in _CASES:
        inputs = fb.seeded(seed)
        for a in inputs:
            a.setflags(write=False)
        _CASES[seed] = inputs
    return _CASES[seed], PARAMS[seed % len(PARAMS)]


def run(seed, form):
    if (seed, form) not in _RUNS:
        inputs, (scale, const) = case(seed)
        _RUNS[(seed, form)] = fb.loop(*inputs, scale, const, form=form)
    return _RUNS[(seed, form)]


def same_fields(a, b):
    assert a.fields.keys() == b.fields.keys()
    for key in a.fields:
        np.testing.assert_array_equal(ref.bits(a.fields[key]), ref.bits(b.fields[key]), err_msg=str(key))


def same_results(a, b):
    assert len(a.states) == len(b.states)
    for t, (x, y) in enumerate(zip(a.states, b.states)):
        np.testing.assert_array_equal(x, y, err_msg=f"round {t + 1}")
    for x, y in zip(a.arrays(), b.arrays()):
        np.testing.assert_array_equal(x, y)
    assert a.before == b.before and a.live == b.live and a.new == b.new


@pytest.mark.parametrize("seed", SEEDS)
def test_the_field_of_the_skeleton_is_the_field_of_the_zeroed_cost_after_every_round(seed):
    a, b = run(seed, "seeds"), run(seed, "zeroed")
    same_fields(a, b)
    same_results(a, b)


@pytest.mark.parametrize("seed", SEEDS)
def test_incremental_is_from_scratch(seed):
    a, c = run(seed, "seeds"), run(seed, "incremental")
    same_fields(a, c)
    same_results(a, c)


@pytest.mark.parametrize("seed", SEEDS)
def test_every_chain_re_adds_to_the_field(seed):
    a = run(seed, "seeds")
    assert a.chains == len(a.branch_label)


def test_the_seeds_have_many_rounds_and_every_parameter_pair():
    rounds = [len(run(seed, "seeds").states) for seed in SEEDS]
    assert sum(r >= 2 for r in rounds) >= 12 and max(rounds) >= 30
    assert {seed % len(PARAMS) for seed in SEEDS} == set(range(len(PARAMS)))
    assert sum(len(run(seed, "seeds").fields) for seed in SEEDS) >= 400


@pytest.mark.parametrize("seed", [1, 7, 9, 19, 25])
def test_the_dijkstra_is_the_relaxation_and_the_breadth_first_search_is_parents_ref(seed):
    """With one seed per label the seeded oracles are the single-source ones of geodesic_ref and parents_ref."""
    (labels, sources, _, _, cost), _ = case(seed)
    graph = fb.Graph(labels, len(sources) - 1, cost)
    seeds = [int(s) for s in sources[1:] if s >= 0]
    field = fb.seeded_field(graph, seeds)
    np.testing.assert_array_equal(ref.bits(field), ref.bits(ref.relaxation(labels, sources, cost)))
    parents, hops, orphans, invalid = fb.seeded_parents(graph, seeds, field)
    want = pref.jacobi(labels, sources, field, cost)
    np.testing.assert_array_equal(parents, want[0])
    np.testing.assert_array_equal(hops, want[1])
    assert (orphans, invalid) == (want[2], want[3]) == (0, 0)


def test_seeds_out_of_range_on_background_or_above_k_are_invalid_and_duplicates_are_not():
    (labels, sources, _, _, cost), _ = case(7)
    k = len(sources) - 1
    graph = fb.Graph(labels, k, cost)
    inside = np.nonzero((labels.reshape(-1) >= 1) & (labels.reshape(-1) <= k))[0]
    background = int(np.nonzero(labels.reshape(-1) == 0)[0][0])
    good, invalid = graph.valid_seeds([int(inside[0]), int(inside[0]), -1, labels.size, background, int(inside[-1])])
    assert good == [int(inside[0]), int(inside[0]), int(inside[-1])] and invalid == 3
    twice = fb.seeded_field(graph, [int(inside[0]), int(inside[0])])
    np.testing.assert_array_equal(ref.bits(twice), ref.bits(fb.seeded_field(graph, [int(inside[0])])))


def test_on_the_thick_t_the_forms_differ():
    inputs = fb.thick_t()
    a = fb.loop(*inputs, 1.25, 0.0)
    single = fb.single_field(*inputs, 1.25, 0.0)
    assert len(a.states) >= 2 and len(single.states) >= 2
    assert a.voxels != single.voxels
    assert set(a.voxels) != set(single.voxels)
    # round 1 is the same path; a later branch leaves the skeleton at another junction
    first = a.offsets[1]
    assert a.voxels[:first] == single.voxels[:single.offsets[1]]
    assert a.branch_junction != single.branch_junction
    same_results(a, fb.loop(*inputs, 1.25, 0.0, form="zeroed"))
    same_results(a, fb.loop(*inputs, 1.25, 0.0, form="incremental"))


@pytest.mark.parametrize("seed", SEEDS)
def test_where_every_label_has_one_path_the_forms_are_equal(seed):
    inputs, _ = case(seed)
    a = fb.loop(*inputs, 1.25, 450.0)
    assert len(a.states) <= 1
    same_results(a, fb.single_field(*inputs, 1.25, 450.0))


@pytest.mark.parametrize("seed", [0, 15, 24])
@pytest.mark.parametrize("max_paths", [1, 3])
def test_max_paths_is_a_prefix(seed, max_paths):
    inputs, (scale, const) = case(seed)
    full, cut = run(seed, "seeds"), fb.loop(*inputs, scale, const, max_paths=max_paths)
    assert len(full.states) > max_paths == len(cut.states)
    for x, y in zip(cut.states, full.states):
        np.testing.assert_array_equal(x, y)
    assert cut.voxels == full.voxels[:cut.offsets[-1]]
