"""
border_targets and the given-target loops with torch.empty and numpy.empty poisoned (-m gpu), in the manner of
tests/test_gpu_poisoned_python.py, whose helper this file uses: every entry point runs twice under 0x00, then
under 0xFF, 0x7F and 0x01; every returned array must have the bits of the 0x00 run, and the 0xFF run is held to
the oracles of tests/border_ref.py and tests/fix_borders_ref.py. Inputs are made and uploaded before the context is
entered: only the wrappers' own allocations are poisoned -- the packed planes, parents and keys of the border
pass, its rows and its counter, the six state words, the rows of every round.

A result that depends on the fill is a read of memory that nothing wrote.
"""

import numpy as np
import pytest

import border_ref
import fix_borders_ref as fx
from aind_exaspim_neuron_segmentation_amd import inference
from test_gpu_dbf import dev  # noqa: F401  (fixture)
from test_gpu_poisoned_python import under_every_fill

pytestmark = pytest.mark.gpu


def test_border_targets(dev, monkeypatch):      # noqa: F811
    labels = border_ref.random_volume(41, (7, 9, 70))
    want = border_ref.brute_force(labels, 5)

    def run():
        return inference.border_targets(labels), inference.border_targets(labels, n_labels=3)

    def hold(out):
        np.testing.assert_array_equal(np.stack(out[0], axis=1), want)
        np.testing.assert_array_equal(np.stack(out[1], axis=1), border_ref.brute_force(labels, 3))

    under_every_fill(monkeypatch, "border_targets", run, hold)


@pytest.mark.parametrize("form", ["single", "loop"])
def test_the_loops_with_given_targets(dev, monkeypatch, form):      # noqa: F811
    labels, sources, dbf, daf, cost = (np.array(a) for a in fx.faces_y())      # its second given round is empty
    rows = border_ref.brute_force(labels, 1)
    given = (rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32))
    field = inference.geodesic_field(labels, sources, cost=cost)
    parents, hops = inference.geodesic_parents(labels, sources, field=field, cost=cost, return_hops=True)
    if form == "single":
        want = fx.single(labels, sources, dbf, daf, parents, hops, 1.25, 0.0, given)
    else:
        want = fx.loop(labels, sources, dbf, daf, cost, 1.25, 0.0, given)
    assert want.empty == [2]
    seen = {}

    def run():
        stats = {}
        if form == "single":
            out = inference.teasar_branches_given(labels, sources, dbf, daf, parents, hops, given, scale=1.25,
                                                  const=0.0, stats=stats)
        else:
            out = inference.teasar_branches_fix_branching_given(labels, sources, dbf, daf, cost, given, scale=1.25,
                                                                const=0.0, stats=stats)
        seen.update(stats)
        return out + (stats["rounds"], stats["empty_rounds"], stats["given_rounds"])

    def hold(out):
        for a, b in zip(out[:6], want.arrays()):
            np.testing.assert_array_equal(a, b)
        assert out[6] == len(want.states) and out[7] == want.empty and out[8] == 3

    under_every_fill(monkeypatch, f"teasar_branches_given[{form}]", run, hold)
    assert seen["vertices"] == want.new and seen["live_labels"] == want.live


def test_skeletonize_fix_borders(dev, monkeypatch):      # noqa: F811
    labels = np.array(fx.faces_touching()[0])

    def run():
        return inference.skeletonize_fix_borders(labels, scale=1.25, const=0.0)

    def hold(out):
        rows = border_ref.brute_force(labels, 2)
        assert sorted(out) == [1, 2]
        for row, (vertices, _, _) in out.items():
            index = set(np.ravel_multi_index(tuple(vertices.T), labels.shape).tolist())
            assert set(rows[rows[:, 0] == row][:, 1].tolist()) <= index      # every cut centre is a vertex

    under_every_fill(monkeypatch, "skeletonize_fix_borders", run, hold)
