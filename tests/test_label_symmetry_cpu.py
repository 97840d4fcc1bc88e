"""
The transforms of tests/label_symmetry.py and the relations of DESIGN 6t, on the CPU oracles (no GPU).

First the transforms themselves: each of the 48 symmetries followed by its inverse is the identity on volumes,
affinities, indices and boxes; embedding followed by cropping is the identity; and, without any oracle, a
transformed affinity array holds the same set of voxel edges with the same values as the one it came from (the
rule "flipped and shifted by one" is checked against voxel pairs, not against itself).

Then every relation the GPU tests ask of the kernels (tests/test_gpu_label_symmetry.py), asserted by the same
functions on the oracles written from the definitions: dbf_ref.brute_force, components_ref.components,
watershed_ref.fragments, region_graph_ref.region_graph, holes_ref.by_components, dbf_ref.segment_table,
pieces_ref.flood_fill and geodesic_ref.heap_dijkstra with geodesic_ref.farthest. All 48 symmetries, seven
offsets with two tails each and the three renamings run on a 5 x 7 x 11 volume. That a relation holds here is what shows that it
follows from the definition and that the transform is coded right, before a kernel is asked to obey it.

Last, the inputs: the bases the GPU tests use are built and their conditions asserted here as well.
"""

import numpy as np
import pytest

import components_ref
import dbf_ref
import geodesic_ref
import holes_ref
import label_symmetry as ls
import pieces_ref
import region_graph_ref
import watershed_ref

SHAPE = (5, 7, 11)
SYMS = pytest.mark.parametrize("sym", ls.SYMMETRIES, ids=ls.name)
OFFSETS = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 0, 4), (2, 3, 1), (3, 1, 2), (1, 0, 0)]
TAILS = [(1, 1, 1), (2, 1, 3)]
TRANSLATIONS = [ls.Translation(o, t, SHAPE) for o in OFFSETS for t in TAILS]


@pytest.fixture(scope="module")
def base():
    return ls.base_inputs(SHAPE, seed=4, dust=6, spans_tiles=False, top=10, block=3, density=0.1)


# ---- the oracles behind the public functions' signatures --------------------------------------------------
def components(threshold, min_size):
    return lambda aff: components_ref.components(aff, threshold, min_size)[0]


def watershed(low, high):
    return lambda aff: watershed_ref.fragments(aff, low, high, 0)[0]


def fill_holes(labels):
    out, stats = holes_ref.by_components(labels)
    return out, stats["filled"], stats["voxels"]


def label_pieces(labels, dust):
    return pieces_ref.flood_fill(labels, int(np.max(labels, initial=0)), dust)[:4]


def geodesic(labels, sources, cost):
    field = geodesic_ref.heap_dijkstra(labels, sources, cost)
    return (field,) + geodesic_ref.farthest(labels, sources, field)


# ---- 1. the transforms are a group, and mean what they say ---------------------------------------------
@SYMS
def test_a_symmetry_and_its_inverse_are_the_identity(sym):
    rng = np.random.default_rng(1)
    v = rng.integers(0, 100, SHAPE).astype(np.int32)
    aff = ls.set_ignored(rng.random((3,) + SHAPE).astype(np.float32), 1.0)
    idx = np.concatenate([[-1], rng.permutation(v.size)[:50]]).astype(np.int32)
    lo = np.stack([rng.integers(0, n, 20) for n in SHAPE], axis=1)
    boxes = np.concatenate([lo, lo + 1 + np.stack([rng.integers(0, n - l) for n, l in zip(SHAPE, lo.T)], axis=1)],
                           axis=1).astype(np.int32)
    boxes[0] = 0
    inv, there = ls.inverse(sym), ls.new_shape(sym, SHAPE)
    assert ls.inverse(inv) == sym and ls.new_shape(inv, there) == SHAPE
    moved = ls.apply_volume(sym, v)
    assert moved.shape == there and moved.flags.c_contiguous
    np.testing.assert_array_equal(ls.apply_volume(inv, moved), v)
    np.testing.assert_array_equal(ls.apply_affinities(inv, ls.apply_affinities(sym, aff)), aff)
    np.testing.assert_array_equal(ls.apply_indices(inv, ls.apply_indices(sym, idx, SHAPE), there), idx)
    np.testing.assert_array_equal(ls.apply_boxes(inv, ls.apply_boxes(sym, boxes, SHAPE), there), boxes)
    # an index follows its voxel, and a box still bounds its voxels
    ok = idx >= 0
    np.testing.assert_array_equal(moved.reshape(-1)[ls.apply_indices(sym, idx, SHAPE)[ok]], v.reshape(-1)[idx[ok]])
    for old, new in zip(boxes[1:], ls.apply_boxes(sym, boxes, SHAPE)[1:]):
        inside = np.zeros(SHAPE, bool)
        inside[tuple(slice(a, b) for a, b in zip(old[:3], old[3:]))] = True
        want = np.zeros(there, bool)
        want[tuple(slice(a, b) for a, b in zip(new[:3], new[3:]))] = True
        np.testing.assert_array_equal(ls.apply_volume(sym, inside), want)


def test_the_symmetries_are_48_different_maps_and_the_generators_13():
    v = np.arange(np.prod(SHAPE)).reshape(SHAPE)
    seen = {(ls.apply_volume(s, v).shape, ls.apply_volume(s, v).tobytes()) for s in ls.SYMMETRIES}
    assert len(seen) == len(ls.SYMMETRIES) == 48
    # six permutations and eight flips, the identity once
    assert len(ls.GENERATORS) == 13 and ls.IDENTITY in ls.GENERATORS


def edge_dict(aff, index_of=lambda idx: idx):
    """{frozenset of the two voxels' linear indices: value} of every edge the convention does not ignore."""
    shape = aff.shape[1:]
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    out = {}
    for c in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[c], hi[c] = slice(0, -1), slice(1, None)
        a, b = index_of(idx[tuple(lo)].ravel()), index_of(idx[tuple(hi)].ravel())
        for u, v, value in zip(a.tolist(), b.tolist(), aff[c][tuple(lo)].ravel().tolist()):
            out[frozenset((u, v))] = value
    return out


@SYMS
def test_transformed_affinities_hold_the_same_voxel_edges(sym):
    aff = ls.watershed_affinities(SHAPE, 5, fill=-7.0)
    moved = ls.apply_affinities(sym, aff, fill=9.0)
    there = ls.new_shape(sym, SHAPE)
    back = lambda idx: ls.apply_indices(ls.inverse(sym), idx, there)      # noqa: E731
    assert edge_dict(moved, back) == edge_dict(aff)
    # the ignored entries of a flipped channel hold the fill; those of the other channels are ignored entries still
    ignored = ls.set_ignored(np.zeros_like(moved, dtype=bool), True)
    assert set(np.unique(moved[ignored]).tolist()) <= {-7.0, 9.0}
    for a in range(3):
        assert (moved[a][ignored[a]] == (9.0 if sym[1][a] else -7.0)).all()
    assert not np.isin(moved[~ignored], (-7.0, 9.0)).any()


@pytest.mark.parametrize("t", TRANSLATIONS, ids=lambda t: t.name)
def test_embedding_then_cropping_is_the_identity(t):
    rng = np.random.default_rng(2)
    v = rng.integers(1, 100, SHAPE).astype(np.int32)
    aff = ls.watershed_affinities(SHAPE, 5)
    idx = np.concatenate([[-1], rng.permutation(v.size)[:50]]).astype(np.int32)
    big = t.volume(v)
    assert big.shape == ls.padded_shape(SHAPE, t.offset, t.tail) and big.flags.c_contiguous
    np.testing.assert_array_equal(t.back(big), v)
    assert (big != 0).sum() == v.size      # the rest is background
    np.testing.assert_array_equal(t.back_indices(t.indices(idx)), idx)
    np.testing.assert_array_equal(big.reshape(-1)[t.indices(idx)[1:]], v.reshape(-1)[idx[1:]])
    # the edges inside the block keep their values; every other edge, those into the padding included, is off
    wide = t.affinities(aff, off=-1.0)
    inside = edge_dict(aff, lambda i: t.indices(i))
    for pair, value in edge_dict(wide).items():
        assert value == inside.get(pair, -1.0)
    assert len(set(inside) - set(edge_dict(wide))) == 0
    boxes = np.array([[0, 0, 0, 0, 0, 0], [1, 2, 3, 2, 4, 9]], dtype=np.int32)
    np.testing.assert_array_equal(t.boxes(boxes), [[0] * 6, list(np.array([1, 2, 3, 2, 4, 9]) + t.offset * 2)])


def test_relabelling_helpers():
    tables = ls.label_maps(9)
    assert set(tables) == {"permutation", "sparse", "one_home_slot"}
    for table in tables.values():
        assert table[0] == 0 and np.unique(table).size == 10 and table.min() == 0
    assert sorted(tables["permutation"][1:]) == list(range(1, 10)) and (tables["permutation"] != np.arange(10)).any()
    assert tables["sparse"].max() > 2 * ls.LDS_SLOTS
    assert (tables["one_home_slot"][1:] % ls.LDS_SLOTS == 1).all()
    table = np.array([0, 7, 3], dtype=np.int32)
    np.testing.assert_array_equal(ls.relabel_volume(np.array([[[0, 1, 2]]], dtype=np.int32), table), [[[0, 7, 3]]])
    np.testing.assert_array_equal(ls.relabel_rows(np.array([5, 6, 8]), table, -1), [5, -1, -1, 8, -1, -1, -1, 6])
    edges, counts = ls.relabel_edges(np.array([[1, 2]]), table, np.array([4]))
    np.testing.assert_array_equal(edges, [[3, 7]])
    np.testing.assert_array_equal(counts, [4])


# ---- 2. the relations on the oracles: symmetries and translations ---------------------------------------
def transforms():
    return [ls.BoxSymmetry(s, SHAPE) for s in ls.SYMMETRIES] + TRANSLATIONS


def test_components_relations(base):
    for dtype in (np.float32, np.float16):
        aff = base["components"].astype(dtype)
        for min_size in ls.MIN_SIZES:
            fn = components(base["threshold"], min_size)
            whole = fn(aff)
            for t in transforms():
                ls.relate_labelling(fn, aff, whole, t)


def test_watershed_and_region_graph_relations(base):
    aff = base["watershed"]
    for low, high in ls.WATERSHED_THRESHOLDS:
        fn = watershed(low, high)
        frags = fn(aff)
        graph = region_graph_ref.region_graph(frags, aff)
        assert len(graph[0]) > 1
        for t in transforms():
            assert watershed_ref.tied_voxels(t.affinities(aff), low, high) == 0
            moved = ls.relate_labelling(fn, aff, frags, t)
            ls.relate_region_graph(region_graph_ref.region_graph, moved, aff, frags, graph, t)


def test_fill_holes_relations(base):
    whole = fill_holes(base["labels"])
    assert whole[1] >= 1
    for t in transforms():
        ls.relate_fill_holes(fill_holes, base["labels"], whole, t)


def test_distance_to_boundary_relations(base):
    labels = base["labels"]
    fields = {border: dbf_ref.brute_force(labels, border) for border in (False, True)}
    assert not np.array_equal(fields[False], fields[True])
    for sym in ls.SYMMETRIES:
        for border in (False, True):
            ls.relate_dbf(dbf_ref.brute_force, labels, fields[border], ls.BoxSymmetry(sym, SHAPE), border)
    for t in TRANSLATIONS:      # the padded volumes are too large for the brute force: the per-label form
        assert ls.relate_dbf_padding(dbf_ref.per_label, labels, fields[True], t) == (2 if min(t.offset) else 1)


def test_segment_table_relations(base):
    labels = base["labels"]
    dbf = dbf_ref.per_label(labels, True)
    whole = dbf_ref.segment_table(labels, dbf)
    for t in transforms():
        ls.relate_segment_table(dbf_ref.segment_table, labels, dbf, whole, t)


def test_label_pieces_relations(base):
    labels = base["labels"]
    counts = []
    for dust in (0, base["dust"]):
        whole = label_pieces(labels, dust)
        counts.append(len(whole[1]))
        for t in transforms():
            ls.relate_pieces(label_pieces, labels, dust, whole, t)
    assert counts[0] - counts[1] == base["facts"]["dust_pieces"] >= 1      # the dust count


def test_geodesic_relations(base):
    labels, sources = base["labels"], base["sources"]
    for cost in (None, base["cost"]):
        whole = geodesic(labels, sources, cost)
        assert np.isinf(whole[0][labels > 0]).any() and (whole[2][1:] >= 0).all()
        for t in transforms():
            ls.relate_geodesic(geodesic, labels, sources, cost, whole, t)


# ---- 3. the relations on the oracles: renamed labels ---------------------------------------------------
@pytest.mark.parametrize("which", ["permutation", "sparse", "one_home_slot"])
def test_renaming_relations(base, which):
    labels, sources, aff = base["labels"], base["sources"], base["watershed"]
    table = ls.label_maps(base["k"])[which]
    for border in (False, True):
        ls.rename_dbf(dbf_ref.per_label, labels, dbf_ref.per_label(labels, border), table, border)
    ls.rename_fill_holes(fill_holes, labels, fill_holes(labels), table)
    dbf = dbf_ref.per_label(labels, True)
    ls.rename_segment_table(dbf_ref.segment_table, labels, dbf, dbf_ref.segment_table(labels, dbf), table)
    graph = region_graph_ref.region_graph(labels, aff)
    ls.rename_region_graph(region_graph_ref.region_graph, labels, aff, graph, table)
    for dust in (0, base["dust"]):
        ls.rename_pieces(label_pieces, labels, dust, label_pieces(labels, dust), table)
    for cost in (None, base["cost"]):
        ls.rename_geodesic(geodesic, labels, sources, cost, geodesic(labels, sources, cost), table)


# ---- 4. the inputs of the GPU tests ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(11, 19, 45), (9, 10, 40)])
def test_the_gpu_bases_have_what_the_relations_need(shape):
    got = ls.base_inputs(shape)      # asserts every condition
    assert got["k"] >= 8 and got["labels"].shape == shape and got["labels"].size < 10**5
    assert not got["labels"].flags.writeable and not got["watershed"].flags.writeable


def test_the_stream_base_has_what_the_relations_need():
    got = ls.stream_inputs()
    assert -(-got["shape"][0] // 8) >= 3      # three slabs at the larger of the two depths
