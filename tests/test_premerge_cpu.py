"""
The size-floor pre-merge without a GPU: the invariants of the oracle in tests/premerge_ref.py on random
graphs whose affinities take 2, 4 or 8 values (so that most maxima tie), and the parts of the feature
that need no device: the C ABI's declarations, binding and refusals, and the Python keyword arguments.
"""

import inspect
import os
import re

import numpy as np
import pytest

import premerge_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.3, 0.6, 0.9, 1.5)
FLOORS = (0, 1, 10, 20, 1000)


def test_the_oracles_invariants_on_tie_heavy_graphs():
    merged_somewhere = several_left_somewhere = False
    for seed, (k, n_edges, levels) in enumerate([(40, 90, 2), (120, 260, 4), (300, 500, 8), (60, 400, 2)]):
        edges, counts, sums, sizes = premerge_ref.random_graph(seed, k, n_edges, levels)
        for threshold in THRESHOLDS:
            m, merge_all = premerge_ref.merge_bound(threshold)
            assert merge_all == (threshold > 1)
            for floor in FLOORS:
                choice = premerge_ref.choices(edges, counts, sums, sizes, threshold, floor)
                root, _ = premerge_ref.roots(choice)   # raises on a cycle
                e2, c2, s2, sizes2, mapping, _ = premerge_ref.one_round(edges, counts, sums, sizes, threshold, floor)
                k2 = len(sizes2) - 1
                # every chosen edge is mergeable, and only tiny fragments choose
                pair = {(int(lo), int(hi)): (int(c), int(s)) for (lo, hi), c, s in zip(edges, counts, sums)}
                for f in range(1, k + 1):
                    if choice[f] != f:
                        c, s = pair[(min(f, choice[f]), max(f, choice[f]))]
                        assert sizes[f] < floor and (merge_all or s > m * c)
                # at most one fragment that is not tiny per set; a set is numbered by its smallest member
                big = np.bincount(mapping[1:][sizes[1:] >= floor], minlength=k2 + 1)
                assert big.max(initial=0) <= 1
                first = [int(np.flatnonzero(mapping == j)[0]) for j in range(1, k2 + 1)]
                assert first == sorted(first) and mapping[0] == 0 and set(mapping[1:]) == set(range(1, k2 + 1))
                assert int(sizes2.sum()) == int(sizes.sum()) and sizes2[0] == sizes[0]
                np.testing.assert_array_equal(sizes2[1:], np.bincount(mapping[1:], sizes[1:], k2 + 1)[1:])
                assert len(e2) <= len(edges) and int(c2.sum()) <= int(counts.sum())
                assert (e2[:, 0] < e2[:, 1]).all() and (s2 <= c2.astype(np.uint64) << np.uint64(24)).all()
                if floor <= 1:   # no fragment is empty
                    np.testing.assert_array_equal(mapping, np.arange(k + 1))
                    for got, want in zip((e2, c2, s2, sizes2), (edges, counts, sums, sizes)):
                        np.testing.assert_array_equal(got, want)
                merged_somewhere |= k2 < k
                several_left_somewhere |= k2 < k and k2 > 1
    assert merged_somewhere and several_left_somewhere


def test_rounds_stop_when_one_merges_nothing_and_compose_their_maps():
    edges, counts, sums, sizes = premerge_ref.random_graph(11, 200, 420, 4)
    graph, composed, history = premerge_ref.rounds(edges, counts, sums, sizes, 0.6, 20, limit=8)
    assert len(history) >= 2 and history[-1] == history[-2] and history[0] < 200
    assert all(a >= b for a, b in zip(history, history[1:]))
    np.testing.assert_array_equal(graph[3][1:], np.bincount(composed[1:], sizes[1:], history[-1] + 1)[1:])
    # a negative floor is the identity as well
    assert premerge_ref.rounds(edges, counts, sums, sizes, 0.6, -5)[2] == [200]


def test_a_line_of_rising_means_is_one_chain():
    k = 50
    edges = np.array([(f, f + 1) for f in range(1, k)], np.int32)
    counts = np.full(k - 1, 3, np.int64)
    sums = np.array([3 * (1000 + f) for f in range(1, k)], np.uint64)
    sizes = np.full(k + 1, 2, np.int64)
    *_, sizes2, mapping, depth = premerge_ref.one_round(edges, counts, sums, sizes, 1.5, 5)
    assert depth == k - 2 and len(sizes2) == 2 and (mapping[1:] == 1).all()   # k - 1, k: the mutual pair


def test_the_header_declares_and_the_binding_binds_the_new_symbols():
    with open(os.path.join(ROOT, "include", "exaspim_affinity.h")) as f:
        header = f.read()
    assert re.search(r"size_t\s+exaspim_region_graph_premerge_workspace_bytes\(int32_t n_labels, "
                     r"int64_t edge_capacity\);", header)
    assert re.search(r"int\s+exaspim_region_graph_premerge\(const int32_t\* edges_dev,", header)
    assert re.search(r"#define\s+EXASPIM_ABI_VERSION\s+5\b", header)
    lib = _native.lib()
    for name in ("exaspim_region_graph_premerge_workspace_bytes", "exaspim_region_graph_premerge"):
        assert name in _native.SIGNATURES and getattr(lib, name).argtypes == _native.SIGNATURES[name][1]
    assert len(_native.SIGNATURES["exaspim_region_graph_premerge"][1]) == 18


def test_workspace_bytes_and_the_refusals_that_come_before_any_launch():
    lib = _native.lib()
    need = lib.exaspim_region_graph_premerge_workspace_bytes(4097, 4096)
    assert need >= 24 * 4096 + 16 * 4098 and need % 256 == 0
    assert lib.exaspim_region_graph_premerge_workspace_bytes(0, 1) > 0
    assert lib.exaspim_region_graph_premerge_workspace_bytes(-1, 4096) == 0 and "n_labels" in _native.last_error()
    for capacity in (0, 3, -4, 1 << 31):
        assert lib.exaspim_region_graph_premerge_workspace_bytes(10, capacity) == 0
        assert "edge_capacity" in _native.last_error()
    # host memory stands in for device memory: every call below is refused before anything is launched
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    good = [p, p, p, p, 4, 3, 0.5, 10, 8, p, p, p, p, p, p, p, need, None]
    def rc(**change):
        args = list(good)
        for i, v in change.items():
            args[int(i[1:])] = v
        return lib.exaspim_region_graph_premerge(*args)
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15):
        assert rc(**{f"a{i}": None}) == -1 and "NULL" in _native.last_error(), i
    assert rc(a4=-1) == -1 and rc(a4=1 << 31) == -1 and rc(a5=-1) == -1
    assert rc(a6=float("nan")) == -1 and "NaN" in _native.last_error()
    assert rc(a8=6) == -1 and rc(a8=0) == -1 and "edge_capacity" in _native.last_error()
    for i, off in ((0, 2), (9, 2), (13, 2), (14, 2), (1, 4), (2, 4), (3, 4), (10, 4), (11, 4), (12, 4), (15, 8)):
        assert rc(**{f"a{i}": p + off}) == -1 and "misaligned" in _native.last_error(), i
    assert rc(a16=lib.exaspim_region_graph_premerge_workspace_bytes(3, 8) - 1) == -3
    assert "workspace" in _native.last_error()


def test_the_keyword_arguments_exist_and_refuse_bad_values_before_any_device_call():
    params = inspect.signature(inference.agglomerate_affinities).parameters
    assert params["premerge_size"].default == 0 and params["premerge_rounds"].default == 4
    assert params["premerge_size"].kind is inspect.Parameter.KEYWORD_ONLY
    params = inspect.signature(inference.premerge_region_graph).parameters
    assert list(params)[:6] == ["edges", "counts", "sums", "sizes", "threshold", "size_floor"]
    assert params["rounds"].default == 4 and params["edge_capacity"].default is None
    assert "changes the segmentation" in inspect.getdoc(inference.agglomerate_affinities).lower()
    aff = np.zeros((3, 2, 2, 2), np.float32)
    for bad in (-1, 2.5, 100.0, "7", None, True):
        with pytest.raises(ValueError):
            inference.agglomerate_affinities(aff, premerge_size=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            inference.agglomerate_affinities(aff, premerge_size=10, premerge_rounds=bad)
    graph = premerge_ref.random_graph(0, 10, 20, 2)
    for bad in (-1, 0.5, 1 << 63):
        with pytest.raises(ValueError):
            inference.premerge_region_graph(*graph, 0.9, bad)
    with pytest.raises(ValueError):
        inference.premerge_region_graph(*graph, 0.9, 10, rounds=0)
    with pytest.raises(ValueError):
        inference.premerge_region_graph(*graph, float("nan"), 10)
