"""
The definition of the watershed fragments against the serial steepest-ascent watershed,
both on the CPU (tests/watershed_ref.py; no GPU, no library):

  - fragments() equals serial_fragments() array for array, numbering included, wherever no voxel has
    two equal maximal eligible edges below high: uniform, box-smoothed and saturated random
    affinities over shapes around the 8 x 8 x 32 tile and four (low, high) pairs. Saturated values
    (exact 0 and 1) tie below high = 2, so those combinations are outside the claim and are held to
    "ties exist" instead;
  - every such case is non-trivial by the oracle itself: more than one fragment, and not what
    connected components give at the smallest threshold above low or at high;
  - hand-built lines along each axis pin the strict low, the inclusive high, NaN, infinities, the
    tie order, the numbering and the size filter with its floor of 1;
  - on affinities quantised to eighths the two differ: the serial algorithm depends on its
    visiting order there, the definition does not;
  - what the library and the Python layer refuse before a device is touched.
"""

import numpy as np
import pytest

import components_ref
import watershed_ref
from watershed_ref import LINES, SHAPES, THRESHOLDS, random_affinities

KINDS = ("uniform", "smooth", "saturated")


def tie_free_by_construction(kind, high):
    # continuous values never repeat among a voxel's six edges; clipped ones repeat at exactly 0 and 1,
    # which stays harmless only while 1 >= high (and 0 is not eligible or never the maximum)
    return kind != "saturated" or high <= 1.0


CLAIMED = [(kind, shape, low, high) for kind in KINDS for shape in SHAPES for low, high in THRESHOLDS
           if tie_free_by_construction(kind, high)]
TIED = [(kind, shape, low, high) for kind in KINDS for shape in SHAPES for low, high in THRESHOLDS
        if not tie_free_by_construction(kind, high)]


@pytest.mark.parametrize("kind,shape,low,high", CLAIMED)
def test_definition_equals_the_serial_watershed_on_tie_free_input(kind, shape, low, high):
    aff = random_affinities(kind, shape)
    assert watershed_ref.tied_voxels(aff, low, high) == 0
    want, k = watershed_ref.serial_fragments(aff, low, high)
    got, got_k = watershed_ref.fragments(aff, low, high, 0)
    assert got.dtype == np.int32 and got_k == k == int(got.max())
    np.testing.assert_array_equal(got, want)
    # not trivial: several fragments, and neither the components of the eligible edges nor those of
    # the edges >= high
    assert k > 1
    above_low = np.nextafter(np.float32(low), np.float32(np.inf))
    assert not np.array_equal(got, components_ref.components(aff, above_low, 0)[0])
    assert not np.array_equal(got, components_ref.components(aff, high, 0)[0])


def test_the_claim_covers_what_the_issue_lists():
    assert len(CLAIMED) == 9 * (4 + 4 + 2) and len(TIED) == 9 * 2
    for kind, shape, low, high in TIED:
        assert watershed_ref.tied_voxels(random_affinities(kind, shape), low, high) > 0


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("case", LINES, ids=[c[0] for c in LINES])
def test_hand_built_lines(case, axis):
    _, values, low, high, min_size, labels = case
    aff = watershed_ref.line_affinities(axis, values)
    got, k = watershed_ref.fragments(aff, low, high, min_size)
    assert got.shape == aff.shape[1:]
    np.testing.assert_array_equal(got.ravel(), labels)
    assert k == max(labels)


def test_the_opposite_tie_order_would_give_other_fragments():
    # voxel 2 has two edges of 0.5: the one to its lower neighbour wins, so it joins {0, 1}; the
    # opposite rule would give {0, 1}, {2, 3, 4}
    got, _ = watershed_ref.fragments(watershed_ref.line_affinities(2, [0.9, 0.5, 0.5, 0.9, 1.0]), 0.1, 0.9999, 0)
    assert got.ravel().tolist() == [1, 1, 1, 2, 2] != [1, 1, 2, 2, 2]
    assert watershed_ref.steepest(watershed_ref.line_affinities(2, [0.9, 0.5, 0.5, 0.9, 1.0]), 0.1).ravel()[2] == 3


def test_numbering_follows_each_fragments_first_voxel_in_three_dimensions():
    aff = random_affinities("uniform", (9, 9, 33))
    got, k = watershed_ref.fragments(aff, 0.3, 0.7, 0)
    first = [int(np.flatnonzero(got.ravel() == label)[0]) for label in range(1, k + 1)]
    assert first == sorted(first)
    filtered, kf = watershed_ref.fragments(aff, 0.3, 0.7, 5)
    sizes = np.bincount(got.ravel())[1:]
    assert kf == int((sizes > 5).sum()) < k
    np.testing.assert_array_equal(filtered != 0, np.isin(got, 1 + np.flatnonzero(sizes > 5)))


def test_float16_is_widened_exactly():
    half = random_affinities("uniform", (9, 9, 33)).astype(np.float16)
    a, ka = watershed_ref.fragments(half, 0.1, 0.9999, 0)
    b, kb = watershed_ref.fragments(half.astype(np.float32), 0.1, 0.9999, 0)
    np.testing.assert_array_equal(a, b)
    assert ka == kb


def test_quantised_affinities_tie_and_the_two_differ():
    aff = (np.floor(random_affinities("uniform", (8, 8, 32)) * 8) / 8).astype(np.float32)
    assert watershed_ref.tied_voxels(aff, 0.1, 0.9999) > 0
    got, k = watershed_ref.fragments(aff, 0.1, 0.9999, 0)
    serial, ks = watershed_ref.serial_fragments(aff, 0.1, 0.9999)
    assert k != ks and not np.array_equal(got, serial)
    # the definition itself does not move: the same call gives the same labels
    np.testing.assert_array_equal(got, watershed_ref.fragments(aff.copy(), 0.1, 0.9999, 0)[0])


# ---- the entry points, as far as they go without a device -------------------------------------------------
def test_abi_refuses_before_a_device_is_touched():
    from aind_exaspim_neuron_segmentation_amd import _native

    lib = _native.lib()
    dims = _native.int3((9, 10, 36))
    need = lib.exaspim_watershed_workspace_bytes(dims)
    assert need == lib.exaspim_components_workspace_bytes(dims) >= 5 * 9 * 10 * 36
    assert lib.exaspim_watershed_workspace_bytes(_native.int3((9, 0, 36))) == 0 and "dims" in _native.last_error()
    assert lib.exaspim_watershed_workspace_bytes(_native.int3((2048, 1024, 1024))) == 0
    fake = 1 << 20          # never dereferenced: every call below is refused before anything is launched
    args = [fake, _native.AFF_F32, dims, 0.1, 0.9999, 0, fake, fake, fake, need, None]

    def refused(code, what, **changes):
        call = list(args)
        names = ["aff", "dtype", "dims", "low", "high", "min_size", "labels", "count", "ws", "need", "stream"]
        for name, value in changes.items():
            call[names.index(name)] = value
        assert lib.exaspim_watershed_fragments(*call) == code, changes
        assert what in _native.last_error(), (changes, _native.last_error())

    for name in ("aff", "labels", "count", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "aff_dtype", dtype=7)
    refused(-1, "dims", dims=_native.int3((0, 10, 36)))
    refused(-1, "NaN", low=float("nan"))
    refused(-1, "NaN", high=float("nan"))
    refused(-1, "misaligned", aff=fake + 2)
    refused(-1, "misaligned", aff=fake + 1, dtype=_native.AFF_F16)
    refused(-1, "misaligned", labels=fake + 2)
    refused(-1, "misaligned", ws=fake + 8)
    refused(-3, "workspace", need=need - 1)


def test_python_layer_refuses_before_a_device_is_touched():
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = np.zeros((3, 4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="no affinities"):
        inference.watershed_fragments(aff[0])
    with pytest.raises(ValueError, match=r"\(3, D, H, W\)"):
        inference.watershed_fragments(aff[:2])
    with pytest.raises(TypeError, match="float32 or float16"):
        inference.watershed_fragments(aff.astype(np.float64))
    with pytest.raises(ValueError, match="basins"):
        inference.agglomerate_affinities(aff, fragments="basins")
    with pytest.raises(ValueError, match="no affinities to score"):
        inference.agglomerate_affinities(aff[0], fragments="watershed")
