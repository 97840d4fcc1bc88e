"""
The slab-by-slab watershed fragments on the CPU: the numpy model of the slab steps
(watershed_stream_ref.py), which carries only what the device carries, is held to the whole-volume oracle
(watershed_ref.fragments), labels and K, for every list of cuts. No GPU and no library needed.
"""

import numpy as np
import pytest

import components_ref
import watershed_ref
import watershed_stream_ref as ref

KINDS = ["uniform", "smooth", "saturated"]
SHAPES = [(5, 6, 7), (9, 9, 33), (17, 17, 65)]      # around the device's 8 x 8 x 32 tile
THRESHOLDS = [(0.1, 0.9999), (0.3, 0.7), (0.0, 2.0)]
BIG = (17, 17, 65)


def cut_lists(depth):
    """None; tile-aligned; one past the tile; ragged; every plane its own slab: those that fit the depth."""
    lists = {"none": [], "aligned": [8], "past": [9], "ragged": [1, 4, 5, 11, 16], "planes": list(range(1, depth))}
    out = {}
    for name, cuts in lists.items():
        cuts = [c for c in cuts if c < depth]
        if name == "none" or (cuts and cuts not in out.values()):
            out[name] = cuts
    return out


CASES = [(kind, shape, name) for kind in KINDS for shape in SHAPES for name in cut_lists(shape[0])]
_WHOLE = {}


def whole(kind, shape, low, high, min_size=0, dtype=np.float32):
    """watershed_ref.fragments of the whole volume, computed once per input and left as it is."""
    key = (kind, shape, low, high, min_size, np.dtype(dtype).name)
    if key not in _WHOLE:
        labels, k = watershed_ref.fragments(affinities(kind, shape, dtype), low, high, min_size)
        labels.setflags(write=False)
        _WHOLE[key] = (labels, k)
    return _WHOLE[key]


def affinities(kind, shape, dtype=np.float32):
    a = watershed_ref.random_affinities(kind, shape)
    if np.dtype(dtype) == np.float16:      # eighths: many equal maxima, every value exact in float16
        a = (np.round(a * 8) / 8).astype(np.float16)
        a.setflags(write=False)
    return a


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("kind,shape,cuts", CASES)
def test_streamed_equals_whole(kind, shape, cuts, low, high):
    aff = affinities(kind, shape)
    want, k = whole(kind, shape, low, high)
    got, k_got, provisional, table, _ = ref.fragments_streamed(aff, low, high, 0, cut_lists(shape[0])[cuts])
    assert k_got == k
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(table[provisional], got)


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("kind,shape,cuts", CASES)
def test_the_masks_equal_the_whole_volumes(kind, shape, cuts, low, high):
    aff = affinities(kind, shape)
    for got, want in zip(ref.slab_on_edges(aff, low, high, cut_lists(shape[0])[cuts]),
                         watershed_ref.on_edges(aff, low, high)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("kind,shape,cuts", CASES)
def test_float16_eighths_with_tied_maxima(kind, shape, cuts, low, high):
    """The tie order, -z first and +z last, is what a seam can get wrong: the carried plane is offered first."""
    aff = affinities(kind, shape, np.float16)
    if shape == BIG:
        assert watershed_ref.tied_voxels(aff, low, high) > 0
    want, k = whole(kind, shape, low, high, dtype=np.float16)
    got, k_got, _, _, _ = ref.fragments_streamed(aff, low, high, 0, cut_lists(shape[0])[cuts])
    assert k_got == k
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("min_size", [1, 2, 5, 40])
@pytest.mark.parametrize("cuts", sorted(cut_lists(BIG[0])))
def test_the_size_filter_sees_whole_fragments(cuts, min_size):
    want, k = whole("smooth", BIG, 0.3, 0.7, min_size)
    got, k_got, _, _, _ = ref.fragments_streamed(affinities("smooth", BIG), 0.3, 0.7, min_size,
                                                 cut_lists(BIG[0])[cuts])
    assert k_got == k
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("cut", [8, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_of_seam_edge_occurs_at_the_cut(kind, cut):
    """From the whole-volume oracle alone: at the cut the (17, 17, 65) inputs have a seam edge that is on only
    through its upper end's choice, one only through its lower end's, one only through >= high, an eligible one
    that stays off, and a fragment on both sides. Without them the cases above would not test the seam."""
    low, high = np.float32(0.3), np.float32(0.7)
    aff = affinities(kind, BIG)
    code = watershed_ref.steepest(aff, low)
    a = aff[0, cut - 1]
    eligible, at_high = a > low, a >= high
    lower, upper = code[cut - 1] == ref.TO_HIGH_Z, code[cut] == ref.TO_LOW_Z
    assert (eligible & ~at_high & ~lower & upper).any()
    assert (eligible & ~at_high & lower & ~upper).any()
    if kind != "smooth":      # a box mean of uniform noise rarely reaches 0.7, and where it does it is a maximum
        assert (eligible & at_high & ~lower & ~upper).any()
    assert (eligible & ~at_high & ~lower & ~upper).any()
    on_z = watershed_ref.on_edges(aff, low, high)[0][cut - 1]
    np.testing.assert_array_equal(on_z, eligible & (at_high | lower | upper))
    labels, _ = whole(kind, BIG, 0.3, 0.7)
    assert ((labels[cut - 1] == labels[cut]) & (labels[cut] > 0) & on_z).any()


def test_the_conservative_marks_cost_ids_not_labels():
    """Below a seam every eligible edge marks its fragment, on or not: with a size filter that gives ids to small
    fragments which exact marks would have left without one, and the labels are the same. (At min_size 0 it costs
    nothing: a voxel with an eligible edge has a steepest edge, so its slab-local fragment has two voxels, or its
    steepest edge crosses a seam and marks it exactly.)"""
    aff = affinities("uniform", BIG)
    low, high, min_size = 0.3, 0.7, 5
    got, k, provisional, table, used = ref.fragments_streamed(aff, low, high, min_size, [8])
    want, k_want = whole("uniform", BIG, low, high, min_size)
    assert k == k_want
    np.testing.assert_array_equal(got, want)
    code = watershed_ref.steepest(aff, np.float32(low))
    a = aff[0, 7]
    eligible = a > np.float32(low)
    off = eligible & ~(a >= np.float32(high)) & (code[7] != ref.TO_HIGH_Z) & (code[8] != ref.TO_LOW_Z)
    assert (provisional[7][eligible] > 0).all()
    dropped = off & (want[7] == 0)      # marked for an edge that stayed off, and too small in the end
    assert dropped.any() and (table[provisional[7][dropped]] == 0).all()
    assert used > k


def test_capacity_overflow():
    aff = affinities("uniform", (9, 9, 33))
    _, _, _, _, used = ref.fragments_streamed(aff, 0.3, 0.7, 0, [4])
    ref.fragments_streamed(aff, 0.3, 0.7, 0, [4], capacity=used)
    with pytest.raises(OverflowError):
        ref.fragments_streamed(aff, 0.3, 0.7, 0, [4], capacity=used - 1)


def test_fragments_are_not_the_streamed_components():
    """The labels differ from the components at 0.5, so no test here can pass on those."""
    aff = affinities("smooth", BIG)
    fragments, k = whole("smooth", BIG, 0.1, 0.9999)
    components, n = components_ref.components(aff, 0.5, 0)
    assert k != n and not np.array_equal(fragments, components)
