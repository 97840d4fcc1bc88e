"""
The label kernels behind segmentation.py on the GPU (-m gpu), held to relations that need no oracle:
the same problem turned, mirrored, moved across the tile grid or given other label ids must give the same answer,
bit for bit, once the answer is taken back. tests/label_symmetry.py holds the transforms and the relations;
tests/test_label_symmetry_cpu.py shows on the CPU oracles that every relation follows from the definitions.

Every function is run once on the untransformed input, and that baseline is held to the function's CPU oracle,
so that a relation between two wrong answers cannot pass. Then
  A. all 48 symmetries of the box, on (11, 19, 45) and (9, 10, 40): x, the row of the kernels, becomes y and z;
  B. seven offsets against the 8 x 8 x 32 tile grid, each with a padded x extent that is a multiple of 4 (the
     16-byte loads stay) and one that is not;
  C. three renamings of the labels: a permutation, a sparse injection into 1 .. 10240, and ids that are all
     equal modulo 2048, the slots of the region graph's table in LDS;
  D. the two streamed labellers on the z-flipped and on the y <-> x transposed volume, at a slab depth of 8 and
     of 5: every seam carries the structure from the other side.
All comparisons are array_equal or bit patterns. Outputs that a "smallest C-order index" rule picks among equals
(peak_index, far_index, and the numbering of components, fragments and pieces) are compared up to that rule under
a symmetry, which does not keep C order, and exactly under a translation and a renaming, which do.
"""

import numpy as np
import pytest
import torch

import components_ref
import dbf_ref
import geodesic_ref
import holes_ref
import label_symmetry as ls
import pieces_ref
import region_graph_ref
import watershed_ref
from aind_exaspim_neuron_segmentation_amd import segmentation

pytestmark = pytest.mark.gpu

BASES = [(11, 19, 45), (9, 10, 40)]
OFFSETS = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 0, 4), (3, 5, 17), (7, 7, 31), (8, 8, 32)]
MAPS = ["permutation", "sparse", "one_home_slot"]
Z_FLIP = ((0, 1, 2), (True, False, False))
YX_SWAP = ((0, 2, 1), (False, False, False))
SLAB_DEPTHS = (8, 5)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=BASES, ids=lambda s: "x".join(map(str, s)))
def base(request):
    return ls.base_inputs(request.param)      # asserts the conditions on the inputs before any kernel runs


def symmetries(shape):
    return [ls.BoxSymmetry(s, shape) for s in ls.SYMMETRIES]


def translations(shape):
    """Every offset with two tails: the padded x extent a multiple of 4, and one more than that."""
    out = []
    for offset in OFFSETS:
        to_four = 4 - (offset[2] + shape[2]) % 4      # 1 .. 4: at least one voxel of padding on the high side
        for tail in ((1, 2, to_four), (2, 1, to_four + 1)):
            t = ls.Translation(offset, tail, shape)
            assert (ls.padded_shape(shape, offset, tail)[2] % 4 == 0) == (tail[2] == to_four) and t.padding < 10**5
            out.append(t)
    return out


def transforms(shape):
    return symmetries(shape) + translations(shape)


# ---- the public functions, numpy in and numpy out ----------------------------------------------------------
def fresh(a):
    """The arrays of a base are read-only and the identity hands them through: upload a copy."""
    return a if a is None or a.flags.writeable else a.copy()


def components(threshold, min_size):
    return lambda aff: segmentation.affinities_to_components(fresh(aff), threshold, min_size)


def watershed(low, high):
    return lambda aff: segmentation.watershed_fragments(fresh(aff), low, high)


def region_graph(labels, aff):
    return segmentation.region_graph(fresh(labels), fresh(aff))


def fill_holes(labels):
    return segmentation.fill_holes(fresh(labels), return_counts=True)


def distance_to_boundary(labels, border):
    return segmentation.distance_to_boundary(fresh(labels), black_border=border)


def segment_table(labels, dbf):
    return segmentation.segment_table(fresh(labels), fresh(dbf))


def label_pieces(labels, dust):
    return segmentation.label_pieces(fresh(labels), dust_threshold=dust)


def geodesic(labels, sources, cost):
    return segmentation.geodesic_field(fresh(labels), fresh(sources), cost=fresh(cost), n_labels=len(sources) - 1,
                                       return_farthest=True)


# ---- baselines: one run on the untransformed input, held to the CPU oracle once ------------------------------
_BASELINES = {}


def baseline(key, run, check):
    if key not in _BASELINES:
        got = run()
        check(got)
        _BASELINES[key] = got
    return _BASELINES[key]


def equal_tuples(want):
    def check(got):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    return check


def components_baseline(inputs, dtype, min_size):
    aff = inputs["components"].astype(dtype)
    fn = components(inputs["threshold"], min_size)
    want = components_ref.components(aff, inputs["threshold"], min_size)[0]
    return aff, fn, baseline(("components", inputs["shape"], np.dtype(dtype).name, min_size), lambda: fn(aff),
                             lambda got: np.testing.assert_array_equal(got, want))


def watershed_baseline(inputs, low, high):
    aff = inputs["watershed"]
    assert watershed_ref.tied_voxels(aff, low, high) == 0
    fn = watershed(low, high)
    want = watershed_ref.fragments(aff, low, high, 0)[0]
    return aff, fn, baseline(("watershed", inputs["shape"], low, high), lambda: fn(aff),
                             lambda got: np.testing.assert_array_equal(got, want))


def dbf_baseline(inputs, border):
    labels = inputs["labels"]
    return baseline(("dbf", inputs["shape"], border), lambda: distance_to_boundary(labels, border),
                    lambda got: np.testing.assert_array_equal(got, dbf_ref.per_label(labels, border)))


def fill_holes_baseline(inputs):
    labels = inputs["labels"]
    want, stats = holes_ref.by_components(labels)
    got = baseline(("holes", inputs["shape"]), lambda: fill_holes(labels),
                   equal_tuples((want, stats["filled"], stats["voxels"])))
    assert got[1] >= 1 and got[2] >= 1
    return got


def segment_table_baseline(inputs):
    labels, dbf = inputs["labels"], dbf_baseline(inputs, True)
    return dbf, baseline(("table", inputs["shape"]), lambda: segment_table(labels, dbf),
                         equal_tuples(dbf_ref.segment_table(labels, dbf)))


def pieces_baseline(inputs, dust):
    labels = inputs["labels"]
    return baseline(("pieces", inputs["shape"], dust), lambda: label_pieces(labels, dust),
                    equal_tuples(pieces_ref.by_label(labels, inputs["k"], dust)[:4]))


def geodesic_baseline(inputs, with_cost):
    labels, sources = inputs["labels"], inputs["sources"]
    cost = inputs["cost"] if with_cost else None

    def check(got):
        want = geodesic_ref.relaxation(labels, sources, cost)
        far_value, far_index = geodesic_ref.farthest(labels, sources, want)
        np.testing.assert_array_equal(ls.bits(got[0]), ls.bits(want))
        np.testing.assert_array_equal(ls.bits(got[1]), ls.bits(far_value))
        np.testing.assert_array_equal(got[2], far_index)
        assert np.isinf(want[labels > 0]).any()

    return cost, baseline(("geodesic", inputs["shape"], with_cost), lambda: geodesic(labels, sources, cost), check)


def graph_baseline(labels, aff, key):
    return baseline(("graph",) + key, lambda: region_graph(labels, aff),
                    equal_tuples(region_graph_ref.region_graph(labels, aff)))


# ---- A and B: the 48 symmetries and the 14 translations ------------------------------------------------------
@pytest.mark.parametrize("min_size", ls.MIN_SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_components(dev, base, dtype, min_size):
    aff, fn, whole = components_baseline(base, dtype, min_size)
    for t in transforms(base["shape"]):
        ls.relate_labelling(fn, aff, whole, t)


@pytest.mark.parametrize("low,high", ls.WATERSHED_THRESHOLDS)
def test_watershed_fragments_and_region_graph(dev, base, low, high):
    aff, fn, frags = watershed_baseline(base, low, high)
    graph = graph_baseline(frags, aff, (base["shape"], low, high))
    assert len(graph[0]) > 1
    for t in transforms(base["shape"]):
        assert watershed_ref.tied_voxels(t.affinities(aff), low, high) == 0
        moved = ls.relate_labelling(fn, aff, frags, t)
        ls.relate_region_graph(region_graph, moved, aff, frags, graph, t)


def test_fill_holes(dev, base):
    whole = fill_holes_baseline(base)
    for t in transforms(base["shape"]):
        ls.relate_fill_holes(fill_holes, base["labels"], whole, t)


@pytest.mark.parametrize("border", [False, True])
def test_distance_to_boundary_under_symmetries(dev, base, border):
    whole = dbf_baseline(base, border)
    for t in symmetries(base["shape"]):
        ls.relate_dbf(distance_to_boundary, base["labels"], whole, t, border)


def test_distance_to_boundary_in_padding(dev, base):
    """Background all around is a black border: the padded volume's field, in either mode, is the volume's
    black-border field. (The plain field is not kept: padding is a boundary the volume did not have.)"""
    whole = dbf_baseline(base, True)
    assert not np.array_equal(whole, dbf_baseline(base, False))
    relations = sum(ls.relate_dbf_padding(distance_to_boundary, base["labels"], whole, t)
                    for t in translations(base["shape"]))
    assert relations == 14 + 8      # four of the seven offsets have padding on every side


def test_segment_table(dev, base):
    dbf, whole = segment_table_baseline(base)
    for t in transforms(base["shape"]):
        ls.relate_segment_table(segment_table, base["labels"], dbf, whole, t)


def test_label_pieces(dev, base):
    kept = []
    for dust in (0, base["dust"]):
        whole = pieces_baseline(base, dust)
        kept.append(len(whole[1]))
        for t in transforms(base["shape"]):
            ls.relate_pieces(label_pieces, base["labels"], dust, whole, t)
    assert kept[0] - kept[1] == base["facts"]["dust_pieces"] >= 1      # the dust count, the same in every run above


@pytest.mark.parametrize("with_cost", [False, True], ids=["euclidean", "cost"])
def test_geodesic_field(dev, base, with_cost):
    cost, whole = geodesic_baseline(base, with_cost)
    for t in transforms(base["shape"]):
        ls.relate_geodesic(geodesic, base["labels"], base["sources"], cost, whole, t)


# ---- C: the same volume under other names ------------------------------------------------------------------
@pytest.fixture(params=MAPS)
def table(request, base):
    tables = ls.label_maps(base["k"])
    assert (tables["permutation"] != np.arange(base["k"] + 1)).any()
    assert tables["sparse"].max() > 2 * ls.LDS_SLOTS and tables["one_home_slot"].max() > 2 * ls.LDS_SLOTS
    assert (tables["one_home_slot"][1:] % ls.LDS_SLOTS == 1).all()
    return tables[request.param]


def test_renamed_distance_to_boundary_and_fill_holes(dev, base, table):
    for border in (False, True):
        ls.rename_dbf(distance_to_boundary, base["labels"], dbf_baseline(base, border), table, border)
    ls.rename_fill_holes(fill_holes, base["labels"], fill_holes_baseline(base), table)


def test_renamed_segment_table(dev, base, table):
    dbf, whole = segment_table_baseline(base)
    ls.rename_segment_table(segment_table, base["labels"], dbf, whole, table)


def test_renamed_region_graph(dev, base, table):
    labels, aff = base["labels"], base["watershed"]
    whole = graph_baseline(labels, aff, (base["shape"], "labels"))
    assert len(whole[0]) >= base["k"]
    ls.rename_region_graph(region_graph, labels, aff, whole, table)


def test_renamed_label_pieces(dev, base, table):
    for dust in (0, base["dust"]):
        ls.rename_pieces(label_pieces, base["labels"], dust, pieces_baseline(base, dust), table)


@pytest.mark.parametrize("with_cost", [False, True], ids=["euclidean", "cost"])
def test_renamed_geodesic_field(dev, base, table, with_cost):
    cost, whole = geodesic_baseline(base, with_cost)
    ls.rename_geodesic(geodesic, base["labels"], base["sources"], cost, whole, table)


# ---- D: streams, reversed ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    inputs = ls.stream_inputs()
    assert all(-(-inputs["shape"][0] // depth) >= 3 for depth in SLAB_DEPTHS)
    return inputs


@pytest.mark.parametrize("sym", [Z_FLIP, YX_SWAP], ids=ls.name)
@pytest.mark.parametrize("slab_depth", SLAB_DEPTHS)
def test_components_streamed_the_other_way(dev, stream, slab_depth, sym):
    t = ls.BoxSymmetry(sym, stream["shape"])
    for min_size in ls.MIN_SIZES:
        aff, _, whole = components_baseline(stream, np.float32, min_size)
        ls.relate_labelling(lambda a: segmentation.affinities_to_components_streaming(
            a, stream["threshold"], min_size, slab_depth=slab_depth), aff, whole, t)


@pytest.mark.parametrize("sym", [Z_FLIP, YX_SWAP], ids=ls.name)
@pytest.mark.parametrize("slab_depth", SLAB_DEPTHS)
def test_watershed_streamed_the_other_way(dev, stream, slab_depth, sym):
    t = ls.BoxSymmetry(sym, stream["shape"])
    for low, high in ls.WATERSHED_THRESHOLDS:
        aff, _, whole = watershed_baseline(stream, low, high)
        ls.relate_labelling(lambda a: segmentation.watershed_fragments_streaming(
            a, low, high, slab_depth=slab_depth), aff, whole, t)
