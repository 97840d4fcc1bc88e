"""
The dominant-edge contraction without a GPU: the invariants of the oracle in tests/dominant_ref.py on
graphs whose means tie everywhere, THE THEOREM against the project's own host merger (agglomerate on the
input equals agglomerate on the oracle-reduced graph composed through the map, table and segment count),
the counter-example that breaks a non-strict rule, the stopping rule, and the parts of the feature that
need no device: the C ABI's declarations, binding and refusals, and the Python keyword arguments.
"""

import inspect
import os
import re

import numpy as np
import pytest

import dominant_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference, segmentation
from premerge_ref import ONE, merge_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# m = 2^23 and 2^22 sit on tied means (1/2, 1/4); 0.6 and 0.9 sit off them; above one merges everything
THRESHOLDS = (0.5, 0.6, 0.75, 0.9, 1.5, 0.0)
SEEDS = range(40)


def seeded_graph(seed):
    rng = np.random.default_rng(7000 + seed)
    k = int(rng.integers(2, 201))
    return dominant_ref.tie_heavy_graph(seed, k, int(rng.integers(1, 3 * k)))


def test_the_oracles_invariants_on_tie_heavy_graphs():
    contracted_somewhere = 0
    for seed in SEEDS:
        edges, counts, sums, sizes = seeded_graph(seed)
        k = len(sizes) - 1
        for threshold in THRESHOLDS:
            m, merge_all = merge_bound(threshold)
            chosen = dominant_ref.dominant_edges(edges, counts, sums, sizes, threshold)
            assert chosen == dominant_ref.dominant_edges_literal(edges, counts, sums, sizes, threshold)
            ends = edges[chosen].ravel().tolist()
            assert len(ends) == len(set(ends))                              # a matching
            assert all(merge_all or int(sums[e]) > m * int(counts[e]) for e in chosen)
            e2, c2, s2, sizes2, mapping = dominant_ref.one_round(edges, counts, sums, sizes, threshold)
            k2 = len(sizes2) - 1
            assert k2 == k - len(chosen) and np.bincount(mapping[1:]).max() <= 2
            first = [int(np.flatnonzero(mapping == j)[0]) for j in range(1, k2 + 1)]
            assert first == sorted(first) and mapping[0] == 0 and set(mapping[1:]) == set(range(1, k2 + 1))
            assert int(sizes2.sum()) == int(sizes.sum()) and sizes2[0] == sizes[0]
            np.testing.assert_array_equal(sizes2[1:], np.bincount(mapping[1:], sizes[1:], k2 + 1)[1:])
            assert len(e2) <= len(edges) and int(c2.sum()) <= int(counts.sum())
            assert (e2[:, 0] < e2[:, 1]).all() and (s2 <= c2.astype(np.uint64) << np.uint64(24)).all()
            if threshold == 0.0:
                np.testing.assert_array_equal(mapping, np.arange(k + 1))
            contracted_somewhere += k2 < k
    assert contracted_somewhere >= len(SEEDS)


@pytest.mark.parametrize("limit", [1, 2, 64])
def test_the_theorem_against_the_host_merger(limit):
    """agglomerate(G) == agglomerate(G reduced) through the map, where ties are everywhere."""
    contracted = 0
    for seed in SEEDS:
        graph = seeded_graph(seed)
        k = len(graph[3]) - 1
        first_round = False
        for threshold in THRESHOLDS:
            for min_size in (0, 30):
                want, want_count = inference.agglomerate(*graph, [threshold], min_size)
                reduced, composed, history = dominant_ref.rounds(*graph, threshold, limit=limit)
                table, count = inference.agglomerate(*reduced, [threshold], min_size)
                np.testing.assert_array_equal(table[composed], want, err_msg=f"seed {seed} T {threshold}")
                assert count == want_count
                first_round |= history[0] < k
        contracted += first_round
    assert 2 * contracted >= len(SEEDS)      # not vacuous: at least half the graphs contract in round one


def counter_example():
    """5-7 and 5-9 tied, 1-9 tied with both, 7-9 low; fragments 1, 5, 7, 9 of nine. At T = 0.6 a mean of
    1/2 merges, and what 7-9 pools with does not: merging 5-7 first would give {5, 7}, {1, 9}."""
    edges = np.array([(1, 9), (5, 7), (5, 9), (7, 9)], np.int32)
    counts = np.array([3, 1, 2, 1], np.int64)
    sums = np.array([3 * (ONE // 2), ONE // 2, ONE, 0], np.uint64)
    return edges, counts, sums, np.full(10, 7, np.int64)


def test_the_counter_example_of_the_non_strict_rule():
    graph = counter_example()
    table, _ = inference.agglomerate(*graph, [0.6], 0)
    assert table[1] == table[5] == table[9] != table[7]       # the greedy: {1, 5, 9}, {7}
    # nothing at fragment 5 may contract in round one, and nothing else does either: every maximum ties
    assert dominant_ref.dominant_edges(*graph, 0.6) == []
    reduced, composed, history = dominant_ref.rounds(*graph, 0.6)
    assert history == [9]
    np.testing.assert_array_equal(composed, np.arange(10))
    # the same with 7-9 on top: it is strictly the best of 7 and of 9 and goes first in both
    edges, counts, sums, sizes = graph
    sums = sums.copy()
    sums[3] = ONE - 1
    assert dominant_ref.dominant_edges(edges, counts, sums, sizes, 0.6) == [3]
    want, n = inference.agglomerate(edges, counts, sums, sizes, [0.6], 0)
    reduced, composed, _ = dominant_ref.rounds(edges, counts, sums, sizes, 0.6)
    got, n2 = inference.agglomerate(*reduced, [0.6], 0)
    np.testing.assert_array_equal(got[composed], want)
    assert n == n2


def test_skipped_rows_neither_dominate_nor_tie():
    edges = np.array([(1, 2), (2, 3), (2, 2), (0, 2), (2, 4), (2, 5)], np.int32)
    counts = np.array([2, 1, 1, 1, 1, 0], np.int64)
    sums = np.array([2 * ONE - 8, ONE - 5, ONE, ONE, ONE, ONE - 4], np.uint64)     # the bad rows tie or beat 1-2
    sizes = np.array([3, 1, 1, 1], np.int64)                                       # K = 3: 4 and 5 are no ids
    e2, c2, s2, sizes2, mapping = dominant_ref.one_round(edges, counts, sums, sizes, 0.9)
    assert mapping.tolist() == [0, 1, 1, 2] and e2.tolist() == [[1, 2]] and sizes2.tolist() == [3, 2, 1]
    assert c2.tolist() == [1] and s2.tolist() == [ONE - 5]


def test_the_stopping_rule_and_the_composed_map():
    assert segmentation._dominant_round_is_last is inference._contract_dominant_on_device.__globals__[
        "_dominant_round_is_last"]
    for k, k_new, last in ((10, 10, True), (10, 9, False), (63, 62, False), (128, 127, True), (128, 126, False),
                           (6400, 6301, True), (6400, 6300, False), (1, 1, True), (0, 0, True)):
        assert segmentation._dominant_round_is_last(k, k_new) is last, (k, k_new)
        assert dominant_ref.is_last(k, k_new) is last
    # a line of rising means contracts one pair per round: with K = 200 the first such round is the last
    k = 200
    edges = np.array([(f, f + 1) for f in range(1, k)], np.int32)
    counts = np.full(k - 1, 3, np.int64)
    sums = np.array([3 * (1000 + f) for f in range(1, k)], np.uint64)
    sizes = np.full(k + 1, 2, np.int64)
    _, composed, history = dominant_ref.rounds(edges, counts, sums, sizes, 1.5)
    assert history == [k - 1] and composed[k] == composed[k - 1] == k - 1
    # with K = 40 (K // 64 = 0) every round removes its one pair until "limit" rounds have run
    _, composed, history = dominant_ref.rounds(edges[:39], counts[:39], sums[:39], sizes[:41], 1.5, limit=5)
    assert history == [39, 38, 37, 36, 35] and (composed[35:] == 35).all()
    # the maps of several rounds compose
    graph = dominant_ref.tie_heavy_graph(3, 150, 300)
    reduced, composed, history = dominant_ref.rounds(*graph, 0.9)
    assert len(history) >= 2 and history == sorted(history, reverse=True) and history[1] < history[0] < 150
    np.testing.assert_array_equal(reduced[3][1:], np.bincount(composed[1:], graph[3][1:], history[-1] + 1)[1:])
    first = [int(np.flatnonzero(composed == j)[0]) for j in range(1, history[-1] + 1)]
    assert first == sorted(first)


def test_the_header_declares_and_the_binding_binds_the_new_symbols():
    with open(os.path.join(ROOT, "include", "exaspim_affinity.h")) as f:
        header = f.read()
    assert re.search(r"size_t\s+exaspim_region_graph_contract_dominant_workspace_bytes\(int32_t n_labels, "
                     r"int64_t edge_capacity\);", header)
    assert re.search(r"int\s+exaspim_region_graph_contract_dominant\(const int32_t\* edges_dev,", header)
    assert re.search(r"#define\s+EXASPIM_ABI_VERSION\s+5\b", header)
    assert "THEOREM" in header and "repeated pairs" in header
    lib = _native.lib()
    for name in ("exaspim_region_graph_contract_dominant_workspace_bytes", "exaspim_region_graph_contract_dominant"):
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert len(_native.SIGNATURES["exaspim_region_graph_contract_dominant"][1]) == 17


def test_workspace_bytes_and_the_refusals_that_come_before_any_launch():
    lib = _native.lib()
    query = lib.exaspim_region_graph_contract_dominant_workspace_bytes
    need = query(4097, 4096)
    assert need >= 24 * 4096 + 12 * 4098 and need % 256 == 0
    assert need < lib.exaspim_region_graph_premerge_workspace_bytes(4097, 4096)      # no doubling buffers
    assert query(0, 1) > 0
    assert query(-1, 4096) == 0 and "n_labels" in _native.last_error()
    for capacity in (0, 3, -4, 1 << 31):
        assert query(10, capacity) == 0 and "edge_capacity" in _native.last_error()
    # host memory stands in for device memory: every call below is refused before anything is launched
    buf = np.full(64, 0x5A5A5A5A5A5A5A5A, np.int64)
    p = buf.ctypes.data
    good = [p, p, p, p, 4, 3, 0.5, 8, p, p, p, p, p, p, p, need, None]

    def rc(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.exaspim_region_graph_contract_dominant(*args)

    for i in (0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14):
        assert rc(**{f"a{i}": None}) == -1 and "NULL" in _native.last_error(), i
    assert rc(a4=-1) == -1 and rc(a4=1 << 31) == -1 and rc(a5=-1) == -1
    assert rc(a6=float("nan")) == -1 and "NaN" in _native.last_error()
    assert rc(a7=6) == -1 and rc(a7=0) == -1 and "edge_capacity" in _native.last_error()
    for i, off in ((0, 2), (8, 2), (12, 2), (13, 2), (1, 4), (2, 4), (3, 4), (9, 4), (10, 4), (11, 4), (14, 8)):
        assert rc(**{f"a{i}": p + off}) == -1 and "misaligned" in _native.last_error(), i
    assert rc(a15=query(3, 8) - 1) == -3 and "workspace" in _native.last_error()
    assert (buf == 0x5A5A5A5A5A5A5A5A).all()


def test_the_keyword_arguments_exist_and_refuse_bad_values_before_any_device_call():
    params = inspect.signature(inference.agglomerate_affinities).parameters
    names = list(params)
    assert params["device_merge_rounds"].default == 0
    assert params["device_merge_rounds"].kind is inspect.Parameter.KEYWORD_ONLY
    assert names.index("device_merge_rounds") == names.index("premerge_rounds") + 1
    assert "bit for bit" in inspect.getdoc(inference.agglomerate_affinities)
    params = inspect.signature(inference.contract_dominant_edges).parameters
    assert list(params)[:5] == ["edges", "counts", "sums", "sizes", "threshold"]
    assert params["rounds"].default == 64 and params["edge_capacity"].default is None
    assert params["rounds"].kind is inspect.Parameter.KEYWORD_ONLY
    aff = np.zeros((3, 2, 2, 2), np.float32)
    for bad in (-1, 2.5, 64.0, "7", None, True):
        with pytest.raises(ValueError):
            inference.agglomerate_affinities(aff, device_merge_rounds=bad)
    graph = dominant_ref.tie_heavy_graph(0, 10, 20)
    for bad in (0, -1, 0.5, 2.0, None, True):
        with pytest.raises(ValueError):
            inference.contract_dominant_edges(*graph, 0.9, rounds=bad)
    with pytest.raises(ValueError):
        inference.contract_dominant_edges(*graph, float("nan"))
    edges, counts, sums, sizes = graph
    with pytest.raises(ValueError, match="2\\^39"):      # the total of host counts: before any device is asked for
        inference.contract_dominant_edges(edges, np.full(len(counts), 1 << 36, np.int64), sums, sizes, 0.9)


@pytest.mark.parametrize("name", ["contract_dominant_edges", "_contract_dominant_on_device", "_device_merged_table"])
def test_the_new_names_are_the_same_objects_under_inference(name):
    assert getattr(inference, name) is getattr(segmentation, name)
    assert getattr(segmentation, name).__module__.endswith(".segmentation")
