"""
tests/border_ref.py against itself (no GPU): the brute force over all pixels and border positions (A) and the
per-component distance transform (B) give the same targets on 40 seeded volumes (k = 5, fill 0.6, the shapes the
GPU tests use) and on the crafted cases, which is DESIGN 6p's claim that e taken on labels equals e taken on
components; and the crafted cases hold what their names say.
"""

import numpy as np
import pytest

import border_ref


@pytest.mark.parametrize("seed", range(40))
def test_the_two_oracles_agree_on_seeded_volumes(seed):
    shape = border_ref.SHAPES[seed % len(border_ref.SHAPES)]
    labels = border_ref.random_volume(seed, shape)
    a, b = border_ref.brute_force(labels, 5), border_ref.by_component(labels, 5)
    np.testing.assert_array_equal(a, b)
    assert len(set(map(tuple, a.tolist()))) == len(a)
    assert (labels.reshape(-1)[a[:, 1]] == a[:, 0]).all()      # a target is a voxel of its label


@pytest.mark.parametrize("name", sorted(border_ref.crafted()))
def test_the_two_oracles_agree_on_the_crafted_cases(name):
    labels, k, on_top = border_ref.crafted()[name]
    a, b = border_ref.brute_force(labels, k), border_ref.by_component(labels, k)
    np.testing.assert_array_equal(a, b)
    if on_top is not None:
        assert len(border_ref.face_targets(labels, k, 0)) == on_top


def test_what_the_crafted_cases_are_for():
    cases = border_ref.crafted()
    labels, k, _ = cases["a two-label checkerboard"]
    for plane, _ in border_ref.faces(labels):
        e = border_ref.e_brute_force(border_ref.foreground(plane, k))
        assert (e == 1).all()      # the tie rule alone decides
    targets = border_ref.brute_force(labels, k)
    assert targets[0].tolist() == [1, 0] and [2, 1] in targets.tolist()
    labels, k, _ = cases["a 2-wide bar"]
    plane = border_ref.foreground(labels[0], k)
    e = border_ref.e_brute_force(plane)
    assert (e[plane > 0] == 1).all() and border_ref.face_targets(labels, k, 0) == [(3, 2 * 12 + 1)]
    labels, k, _ = cases["a blob with a unique maximum"]
    e = border_ref.e_brute_force(border_ref.foreground(labels[0], k))
    assert (e == e.max()).sum() == 1 and border_ref.face_targets(labels, k, 0) == [(4, 5 * 13 + 6)]
    labels, k, _ = cases["an edge and a corner"]
    assert border_ref.brute_force(labels, k).tolist() == [[1, 0], [2, 3], [3, (3 * 5 + 2) * 6 + 5]]
    labels, k, _ = cases["labels <= 0 and > K ignored"]
    assert border_ref.brute_force(labels, k).tolist() == [[2, 2 * 30 + 1 * 6 + 1 + 7]]
    assert border_ref.brute_force(cases["an empty volume"][0], 3).shape == (0, 2)


def test_the_seam_property_of_the_oracle():
    """Both sides of a cut see the same plane, so they pick the same voxels."""
    volume = border_ref.random_volume(7, (6, 9, 20))
    w = volume.shape[2]
    for s in (1, 7, 18):
        a, b = volume[:, :, :s + 1], volume[:, :, s:]
        left = {(l, v // (s + 1) * w + s) for l, v in border_ref.face_targets(a, 5, 5)}
        right = {(l, v // (w - s) * w + s) for l, v in border_ref.face_targets(b, 5, 4)}
        assert left == right and left
