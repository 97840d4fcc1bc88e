"""
The method of the slab-by-slab region graph on the CPU: tests/region_graph_stream_ref.py --
per-slab graphs of provisional ids, seam contributions from a carried plane of ids and a carried plane
of quantised z affinities, keys translated through the id -> fragment table with equal ends dropped and
equal keys pooled -- gives, bit for bit, the whole volume's region graph of the final fragments, and the
composed table segment[fragment[id]] gives region_graph_ref.agglomerate_affinities. The figures pinned
here say that every case exercises all three mechanisms; the GPU tests rely on the same cases.
"""

import numpy as np
import pytest

import components_ref
import region_graph_ref
import region_graph_stream_ref

RAGGED = [1, 2, 3, 9, 20, 22]
CUTS = {"aligned": lambda d: [8, 16], "ragged": lambda d: RAGGED, "planes": lambda d: list(range(1, d))}

# shape, fragment threshold, cuts: K, final edges, provisional ids, provisional keys, dropped and pooled in
# translation, seam contributions
ROWS = [
    ((23, 37, 71), 0.6, "aligned", (836, 1066, 1367, 2535, 1167, 302, 4783)),
    ((23, 37, 71), 0.6, "ragged", (836, 1066, 3373, 10708, 8069, 1573, 14133)),
    ((23, 37, 71), 0.6, "planes", (836, 1066, 11739, 50825, 44907, 4852, 52172)),
    ((23, 37, 71), 0.75, "aligned", (6116, 22796, 7288, 27667, 1839, 3032, 3590)),
    ((23, 37, 71), 0.75, "ragged", (6116, 22796, 9751, 35374, 5703, 6875, 10377)),
    ((23, 37, 71), 0.75, "planes", (6116, 22796, 19574, 66458, 22006, 21656, 38858)),
    ((24, 40, 72), 0.6, "aligned", (937, 1179, 1529, 2832, 1280, 373, 5217)),
    ((24, 40, 72), 0.6, "ragged", (937, 1179, 3532, 11117, 8323, 1615, 15615)),
    ((24, 40, 72), 0.6, "planes", (937, 1179, 13606, 59245, 52542, 5524, 59827)),
    ((24, 40, 72), 0.75, "aligned", (7134, 27024, 8430, 32236, 2024, 3188, 3917)),
    ((24, 40, 72), 0.75, "ragged", (7134, 27024, 11170, 41205, 6267, 7914, 11642)),
    ((24, 40, 72), 0.75, "planes", (7134, 27024, 22651, 77047, 24815, 25208, 44707)),
]

_WHOLE = {}


def random_affinities(shape):
    a = np.random.default_rng(5).random((3,) + shape).astype(np.float32)
    a.setflags(write=False)
    return a


def whole(shape, fragment_threshold):
    """(aff, fragments, K, graph) of the whole volume, computed once."""
    key = (shape, fragment_threshold)
    if key not in _WHOLE:
        aff = random_affinities(shape)
        fragments, k = components_ref.components(aff, fragment_threshold, 0)
        _WHOLE[key] = (aff, fragments, k, region_graph_ref.region_graph(fragments, aff, k))
    return _WHOLE[key]


def assert_same(got, want):
    for g, w, name in zip(got, want, ("edges", "counts", "sums", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("shape,fragment_threshold,cuts,figures", ROWS)
def test_the_model_equals_the_whole_volume_graph(shape, fragment_threshold, cuts, figures):
    aff, fragments, k, want = whole(shape, fragment_threshold)
    graph, got_k, acc, dropped, pooled, final = region_graph_stream_ref.fragments_streamed(
        aff, fragment_threshold, CUTS[cuts](shape[0]))
    assert got_k == k
    np.testing.assert_array_equal(final, fragments)
    assert_same(graph, want)
    ids = int(np.flatnonzero(acc.sizes_by_id).max())
    got = (k, len(graph[0]), ids, acc.keys.size, dropped, pooled, acc.seam_contributions)
    print("K, E, provisional ids, provisional keys, dropped, pooled, seam contributions:", got)
    assert got == figures
    # all three mechanisms: seam edges, edges inside one fragment, edges that pool
    assert acc.seam_contributions > 0 and dropped > 0 and pooled > 0 and acc.keys.size > len(graph[0])
    assert acc.keys.size - dropped - pooled == len(graph[0])
    assert int(acc.sizes_by_id.sum()) == int(np.prod(shape))


def test_the_composed_table_reproduces_agglomerate_affinities():
    partly = False
    for shape in ((9, 10, 37), (17, 8, 33)):
        aff = random_affinities(shape)
        for thresholds, min_size in (([0.55], 0), ([0.5, 0.6], 0), ([0.6], 10), ([0.9], 0)):
            want = region_graph_ref.agglomerate_affinities(aff, thresholds, min_size, 0.75)
            for slab_depth in (1, 4, 7):
                got, composed, s, k = region_graph_stream_ref.agglomerate_affinities_streamed(
                    aff, thresholds, min_size, 0.75, slab_depth)
                assert got.dtype == np.int32 and composed[0] == 0
                np.testing.assert_array_equal(got, want)
                assert s == int(want.max(initial=0))
                partly = partly or 1 < s < k
    assert partly


def test_finish_with_a_table_that_is_no_fragment_table():
    """Ids beyond the table and entries outside 0 .. n_labels are background; the accumulator survives."""
    shape, id_capacity, n_labels = (9, 10, 37), 30, 7
    rng = np.random.default_rng(43)
    labels = rng.integers(-2, 41, shape).astype(np.int32)
    aff = random_affinities(shape)
    acc = region_graph_stream_ref.accumulate(labels, aff, list(range(1, 9)), id_capacity)
    for seed in (1, 2):
        table = np.random.default_rng(seed).integers(0, n_labels + 3, 25).astype(np.int32)
        table[0] = 0      # id 0 is the background of every table: it forms no edge whatever it maps to
        ok = (labels >= 0) & (labels <= id_capacity)
        inside = ok & (labels < table.size)
        mapped = np.where(inside, table[np.clip(labels, 0, table.size - 1)], 0)
        mapped = np.where(mapped > n_labels, 0, mapped)
        mapped = np.where(ok, mapped, -1).astype(np.int32)
        got, _, _ = region_graph_stream_ref.finish(acc, table, n_labels)
        assert_same(got, region_graph_ref.region_graph(mapped, aff, n_labels))
