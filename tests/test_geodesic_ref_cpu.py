"""
The two CPU oracles of geodesic_field (tests/geodesic_ref.py) held to each other, without a GPU: the heap
Dijkstra in numpy.float32 and the vectorised relaxation agree as int32 bit patterns on 48 seeded volumes of
side 1 to 10 in both modes (costs with 0, -0.0, +inf, NaN and negatives), both agree with scipy's
csgraph.dijkstra in float64 on the same graph to a relative 1e-5 on the finite values (which checks the
weights and the graph, nothing more), and the hand-built cases give what the definition says.
"""

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

import geodesic_ref as ref

SEEDS = list(range(48))


def scipy_field(labels, sources, cost):
    """float64 distances by scipy on the same graph; zero-weight steps are kept by a tiny positive stand-in."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    shape = labels.shape
    k = len(sources) - 1
    sources, _ = ref.valid_sources(labels, sources)
    joined = np.where((labels >= 1) & (labels <= k), labels, 0)
    index = np.arange(labels.size).reshape(shape)
    weight = None if cost is None else ref.entering_weight(cost).astype(np.float64)
    rows, cols, vals = [], [], []
    for o in ref.OFFSETS:
        src = tuple(slice(max(0, -c), s - max(0, c)) for c, s in zip(o, shape))
        dst = tuple(slice(max(0, c), s - max(0, -c)) for c, s in zip(o, shape))
        same = (joined[src] == joined[dst]) & (joined[src] > 0)
        step = (np.full(shape, float(ref.STEP[sum(c != 0 for c in o)])) if weight is None else weight)[dst]
        same &= np.isfinite(step)
        rows.append(index[src][same])
        cols.append(index[dst][same])
        vals.append(np.maximum(step[same], 1e-300))      # csgraph drops explicit zeros
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                       shape=(labels.size, labels.size)).tocsr()
    out = np.where(labels > 0, np.inf, 0.0).reshape(-1)
    starts = [int(s) for s in sources[1:] if s >= 0]
    if starts:
        dist = dijkstra(graph, directed=True, indices=starts)
        for s, row in zip(starts, dist):
            mine = joined.reshape(-1) == joined.reshape(-1)[s]
            out[mine] = row[mine]
    return out.reshape(shape)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_two_oracles_agree_bit_for_bit_and_with_scipy(seed):
    labels, sources, cost = ref.seeded_case(seed)
    a = ref.heap_dijkstra(labels, sources, cost)
    b = ref.relaxation(labels, sources, cost)
    assert a.dtype == b.dtype == np.float32 and a.shape == labels.shape
    np.testing.assert_array_equal(ref.bits(a), ref.bits(b))
    assert not np.isnan(a).any() and (a >= 0).all() and (ref.bits(a) >= 0).all()      # never -0.0
    assert (a[labels <= 0] == 0).all() and np.isinf(a[labels > len(sources) - 1]).all()
    want = scipy_field(labels, sources, cost)
    np.testing.assert_array_equal(np.isfinite(a), np.isfinite(want))
    finite = np.isfinite(a)
    np.testing.assert_allclose(a[finite], want[finite], rtol=1e-5, atol=1e-30)


def test_the_seeds_cover_both_modes_and_the_special_costs():
    cases = [ref.seeded_case(seed) for seed in SEEDS]
    assert sum(c[2] is None for c in cases) >= 20 and sum(c[2] is not None for c in cases) >= 20
    costs = np.concatenate([c[2].reshape(-1) for c in cases if c[2] is not None])
    assert (costs == 0).any() and np.signbit(costs[costs == 0]).any() and not np.signbit(costs[costs == 0]).all()
    assert np.isposinf(costs).any() and np.isnan(costs).any() and (costs < 0).any()
    assert {c[0].shape[0] for c in cases} >= {1, 10} and any(min(c[0].shape) == 1 for c in cases)
    assert any((c[1][1:] == -1).any() and (c[0] == len(c[1]) - 1).any() for c in cases)      # present, no source
    fields = [ref.relaxation(*c) for c in cases]
    assert sum(np.isinf(f).any() for f in fields) >= 10 and sum((f[np.isfinite(f)] > 3).any() for f in fields) >= 10


@pytest.mark.parametrize("oracle", [ref.heap_dijkstra, ref.relaxation])
def test_hand_built_cases(oracle):
    row = np.ones((1, 1, 9), dtype=np.int32)
    np.testing.assert_array_equal(oracle(row, np.array([-1, 0], dtype=np.int32))[0, 0], np.arange(9, dtype=np.float32))
    np.testing.assert_array_equal(oracle(row, np.array([-1, 4], dtype=np.int32))[0, 0],
                                  np.abs(np.arange(9) - 4).astype(np.float32))

    diag = np.zeros((7, 7, 7), dtype=np.int32)
    diag[np.arange(7), np.arange(7), np.arange(7)] = 1
    want, total = [], np.float32(0)
    for _ in range(7):
        want.append(total)
        total = np.float32(total + ref.SQRT3)
    got = oracle(diag, np.array([-1, 0], dtype=np.int32))
    np.testing.assert_array_equal(ref.bits(got[np.arange(7), np.arange(7), np.arange(7)]),
                                  ref.bits(np.array(want, dtype=np.float32)))
    assert ref.bits(np.array([ref.SQRT2, ref.SQRT3])).tolist() == [0x3FB504F3, 0x3FDDB3D7]
    assert ref.SQRT2 == np.float32(np.sqrt(2.0)) and ref.SQRT3 == np.float32(np.sqrt(3.0))

    pieces = np.zeros((3, 3, 12), dtype=np.int32)
    pieces[1, 1, :4] = 2
    pieces[1, 1, 6:] = 2      # the same id, two voxels away
    got = oracle(pieces, np.array([-1, -1, 36 + 12 + 1], dtype=np.int32))
    np.testing.assert_array_equal(got[1, 1, :4], [1, 0, 1, 2])
    assert np.isposinf(got[1, 1, 6:]).all() and (got[pieces == 0] == 0).all()
    value, index = ref.farthest(pieces, np.array([-1, -1, 49], dtype=np.int32), got)
    assert value.tolist() == [0, 0, 2] and index.tolist() == [-1, -1, 36 + 12 + 3]

    # cost mode: the cost of the voxel entered; a zero-cost run ties; a NaN voxel walls the rest off
    cost = np.array([5, 2, 0, -0.0, 3, np.nan, 1], dtype=np.float32).reshape(1, 1, 7)
    got = oracle(np.ones((1, 1, 7), dtype=np.int32), np.array([-1, 0], dtype=np.int32), cost)
    np.testing.assert_array_equal(ref.bits(got[0, 0]), ref.bits(np.array([0, 2, 2, 2, 5, np.inf, np.inf], dtype=np.float32)))


def test_invalid_sources_are_counted_and_ignored():
    labels = np.zeros((2, 3, 4), dtype=np.int32)
    labels[0] = 1
    labels[1] = 2
    sources = np.array([7, 12, 24, 5], dtype=np.int32)      # row 0 ignored; 12 is label 2; 24 out of range; 5 is label 1
    cleaned, invalid = ref.valid_sources(labels, sources)
    assert cleaned.tolist() == [-1, -1, -1, -1] and invalid == 3
    field = ref.relaxation(labels, sources)
    assert np.isposinf(field).all()
    value, index = ref.farthest(labels, sources, field)
    assert value.tolist() == [0, 0, 0, 0] and index.tolist() == [-1, -1, -1, -1]
