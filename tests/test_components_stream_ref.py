"""
The slab-by-slab algorithm of DESIGN 6d, as a numpy model (tests/components_stream_ref.py), against
the whole-volume oracle (tests/components_ref.py), without a GPU: the singleton rule, the numbering
argument and the rationing of provisional ids are pinned here independently of the kernels.
"""

import numpy as np
import pytest

import components_ref
import components_stream_ref

SHAPE = (23, 37, 71)
CUTS = {"aligned": [8, 16], "ragged": [1, 2, 3, 9, 20, 22], "planes": list(range(1, SHAPE[0]))}


@pytest.fixture(scope="module")
def aff():
    a = np.random.default_rng(5).random((3,) + SHAPE).astype(np.float32)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def whole(aff):
    return {(t, m): components_ref.components(aff, t, m) for t in (0.6, 0.8) for m in (0, 100)}


@pytest.mark.parametrize("cuts", sorted(CUTS))
@pytest.mark.parametrize("min_size", [0, 100])
@pytest.mark.parametrize("threshold", [0.6, 0.8])
def test_model_equals_whole_volume_oracle(aff, whole, threshold, min_size, cuts):
    want, k = whole[(threshold, min_size)]
    got, got_k, provisional, table = components_stream_ref.components_streamed(aff, threshold, min_size, CUTS[cuts])
    assert got_k == k
    np.testing.assert_array_equal(got, want)
    assert table[0] == 0 and provisional.max() == table.size - 1


def test_model_foreground_mode_and_lone_voxels():
    p = np.random.default_rng(17).random((12, 20, 40)).astype(np.float32)
    for min_size in (0, 1, 10):
        want, k = components_ref.components(p, 0.6, min_size)
        for cuts in ([5], list(range(1, 12))):
            got, got_k, _, _ = components_stream_ref.components_streamed(p, 0.6, min_size, cuts)
            assert got_k == k
            np.testing.assert_array_equal(got, want)


def test_model_singletons_joined_only_by_seam_edges():
    aff = np.zeros((3, 6, 3, 5), np.float32)
    aff[0, 0:5, 1, 2] = 1.0      # one z column of 6 voxels
    aff[0, 2:4, 2, 4] = 1.0      # one of 3
    cuts = list(range(1, 6))
    for min_size, k in ((0, 2), (3, 1), (6, 0)):
        want, want_k = components_ref.components(aff, 0.5, min_size)
        got, got_k, provisional, _ = components_stream_ref.components_streamed(aff, 0.5, min_size, cuts)
        assert got_k == want_k == k
        np.testing.assert_array_equal(got, want)
    # only voxels with a seam edge were given an id: 6 + 3 of the 90
    assert np.count_nonzero(provisional) == 9


def test_model_capacity():
    aff = np.random.default_rng(5).random((3, 6, 9, 11)).astype(np.float32)
    with pytest.raises(OverflowError):
        components_stream_ref.components_streamed(aff, 0.8, 0, [3], capacity=4)
