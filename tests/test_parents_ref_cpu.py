"""
The two CPU oracles of geodesic_parents (tests/parents_ref.py) held to each other and to the properties the
definition promises, without a GPU: the breadth-first search and the Jacobi rounds agree on 48 seeded volumes in
both modes and on the variant whose costs are absorbed; every parent is adjacent, of the same label and one hop
nearer; every chain has hops steps and re-summing the weights along it gives the field's bits; a heap Dijkstra
that records predecessors yields only tight edges; and the plateau volumes of the GPU tests do hold voxels
whose parent has the same field bits, so that those cases are not vacuous.
"""

import heapq

import numpy as np
import pytest

import geodesic_ref as ref
import parents_ref as pref

_CASES = {}


def case(key):
    """(labels, sources, cost, field, parents, hops) of a seed or a named volume, computed once."""
    if key not in _CASES:
        if key == "line":
            labels, sources, cost = pref.plateau_line()
        elif key == "slab":
            labels, sources, cost = pref.plateau_slab()
        elif isinstance(key, tuple):
            labels, sources, cost = pref.absorbed_case(key[1])
        else:
            labels, sources, cost = ref.seeded_case(key)
        field = ref.relaxation(labels, sources, cost)
        parents, hops, orphans, invalid = pref.jacobi(labels, sources, field, cost)
        assert orphans == 0 and invalid == 0
        for a in (labels, sources, field, parents, hops) + (() if cost is None else (cost,)):
            a.setflags(write=False)
        _CASES[key] = (labels, sources, cost, field, parents, hops)
    return _CASES[key]


ABSORBED = [("absorbed", seed) for seed in range(1, 48, 8)]      # a quarter of the cost cases


@pytest.mark.parametrize("key", list(range(48)) + ABSORBED + ["line", "slab"])
def test_the_two_oracles_agree(key):
    labels, sources, cost, field, parents, hops = case(key)
    a_parents, a_hops, a_orphans, a_invalid = pref.breadth_first(labels, sources, field, cost)
    assert (a_orphans, a_invalid) == (0, 0)
    np.testing.assert_array_equal(a_hops, hops)
    np.testing.assert_array_equal(a_parents, parents)
    assert parents.dtype == np.int32 and hops.dtype == np.int32


@pytest.mark.parametrize("key", list(range(48)) + ABSORBED + ["line", "slab"])
def test_what_the_definition_promises(key):
    labels, sources, cost, field, parents, hops = case(key)
    shape = labels.shape
    k = len(sources) - 1
    valid, _ = ref.valid_sources(labels, sources)
    weight = None if cost is None else ref.entering_weight(cost)
    flat_p, flat_h, flat_l, flat_d = parents.reshape(-1), hops.reshape(-1), labels.reshape(-1), field.reshape(-1)
    # hops exist exactly where the field is finite on a label with a source
    joined = (labels >= 1) & (labels <= k)
    np.testing.assert_array_equal(hops >= 0, joined & np.isfinite(field))
    np.testing.assert_array_equal(parents >= 0, hops >= 0)
    for row in range(1, k + 1):
        if valid[row] >= 0:
            assert flat_h[valid[row]] == 0 and flat_p[valid[row]] == valid[row]
    assert set(np.nonzero(flat_h == 0)[0]) == {int(s) for s in valid[1:] if s >= 0}
    for v in np.nonzero(flat_h >= 1)[0]:
        u = flat_p[v]
        cv, cu = np.unravel_index(v, shape), np.unravel_index(u, shape)
        assert u != v and max(abs(int(a) - int(b)) for a, b in zip(cv, cu)) == 1      # adjacent
        assert flat_l[u] == flat_l[v] and flat_h[u] == flat_h[v] - 1
    # every chain has hops steps, and re-summing along it gives the field's bits at every voxel of it
    ends = np.nonzero(flat_h >= 0)[0]
    for v in ends[np.argsort(-flat_h[ends], kind="stable")][:40]:      # the longest chains cover the others
        path = pref.walk(parents, hops, int(v))
        assert len(path) == flat_h[v] + 1 and path[-1] == v and flat_h[path[0]] == 0
        total = np.float32(0)
        for a, b in zip(path, path[1:]):
            ca, cb = np.unravel_index(a, shape), np.unravel_index(b, shape)
            step = ref.STEP[sum(int(x != y) for x, y in zip(ca, cb))] if weight is None else weight.reshape(-1)[b]
            total = np.float32(total + step)
            assert total.view(np.int32) == flat_d[b].view(np.int32)


@pytest.mark.parametrize("seed", list(range(24)) + [1 + 8 * i for i in range(3)])
def test_a_heap_dijkstra_that_records_predecessors_yields_only_tight_edges(seed):
    """The definition is a Dijkstra tree wherever ties are absent: every recorded predecessor is a tight one."""
    labels, sources, cost, field, parents, hops = case(seed)
    shape = labels.shape
    k = len(sources) - 1
    valid, _ = ref.valid_sources(labels, sources)
    joined = np.where((labels >= 1) & (labels <= k), labels, 0)
    w = None if cost is None else ref.entering_weight(cost)
    d = np.where(labels > 0, ref.INF, np.float32(0)).astype(np.float32)
    before = {}
    for row in range(1, k + 1):
        if valid[row] < 0:
            continue
        start = tuple(int(c) for c in np.unravel_index(valid[row], shape))
        d[start] = 0
        heap, done = [(np.float32(0), start)], set()
        while heap:
            du, u = heapq.heappop(heap)
            if u in done:
                continue
            done.add(u)
            for o in ref.OFFSETS:
                v = (u[0] + o[0], u[1] + o[1], u[2] + o[2])
                if min(v) < 0 or any(c >= s for c, s in zip(v, shape)) or joined[v] != row or v in done:
                    continue
                step = ref.STEP[sum(c != 0 for c in o)] if w is None else w[v]
                dv = np.float32(du + step)
                if dv < d[v]:
                    d[v] = dv
                    before[v] = (u, step)
                    heapq.heappush(heap, (dv, v))
    np.testing.assert_array_equal(ref.bits(d), ref.bits(field))
    assert len(before) == int((hops >= 1).sum())
    for v, (u, step) in before.items():
        assert np.float32(field[u] + step).view(np.int32) == field[v].view(np.int32)      # tight
        assert hops[u] >= 0 and hops[v] <= hops[u] + 1      # hops is the least count over tight chains


@pytest.mark.parametrize("key", ["line", "slab"] + ABSORBED[:2])
def test_the_plateau_cases_hold_a_plateau(key):
    labels, sources, cost, field, parents, hops = case(key)
    count = pref.plateau_count(parents, field)
    print(f"{key}: {int((hops >= 1).sum())} voxels with parents, {count} with the parent's field bits")
    if key in ("line", "slab"):
        assert count >= 1
        assert np.float32(pref.BIG + np.float32(1)) == pref.BIG
    if key == "line":      # the parents march towards +x, across x = 63 | 64 and 31 | 32; x - 1 would make 2-cycles
        n = labels.shape[2]
        x = np.arange(n - 1)
        np.testing.assert_array_equal(parents[1, 1, :n - 1], np.ravel_multi_index((1, 1, x + 1), labels.shape))
        np.testing.assert_array_equal(hops[1, 1], n - 1 - np.arange(n))
        assert count == n - 2      # x = 0 .. n - 3: the parent x + 1 holds 2^25 as well
        assert (field[1, 1, :n - 1] == pref.BIG).all()


def test_a_field_of_another_cost_has_orphans():
    labels, sources, cost, field, parents, hops = case(1)
    other = np.where(np.isfinite(cost) & (cost > 0), cost * np.float32(1.37), cost).astype(np.float32)
    a = pref.breadth_first(labels, sources, field, other)
    b = pref.jacobi(labels, sources, field, other)
    assert a[2] == b[2] > 0
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_a_source_whose_field_is_not_zero_is_invalid():
    labels, sources, cost, field, parents, hops = case(2)
    row = next(r for r in range(1, len(sources)) if sources[r] >= 0)
    spoiled = field.copy()
    spoiled.reshape(-1)[sources[row]] = 1.0
    a = pref.breadth_first(labels, sources, spoiled, cost)
    b = pref.jacobi(labels, sources, spoiled, cost)
    assert a[3] == b[3] == 1 and a[2] == b[2]
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert (b[1][labels == row] == -1).all()
