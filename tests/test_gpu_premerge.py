"""
exaspim_region_graph_premerge, inference.premerge_region_graph and agglomerate_affinities(premerge_size=...)
on the GPU (-m gpu), array for array against the Python-integer oracle of tests/premerge_ref.py: the edge
list after sorting by (lo, hi), map, sizes', K' and E' exact.

The graphs sit where the kernels can go wrong: fragment counts around the scan's block of 2048, chains as
long as the graph (pointer doubling), thousands of adds on one sizes' word and on one table slot, ties
everywhere, the merge bound hit exactly, counts up to 2^27 whose cross products need the high words of the
128-bit comparison and whose pooled sums pass 2^61. Every direct call runs with guard words behind every
buffer and a workspace pre-filled with 0xFF. End to end the chain is also held to the oracles at 16 115
watershed fragments (region_graph_ref.agglomerate_fast after premerge_ref.rounds).
"""

from fractions import Fraction

import numpy as np
import pytest
import torch

import premerge_ref
import region_graph_ref
import watershed_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference

pytestmark = pytest.mark.gpu

ONE = 1 << 24
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def capacity_for(n_edges):
    return 1 << max(2 * n_edges - 1, 0).bit_length()


class Call:
    """One exaspim_region_graph_premerge call: every buffer with GUARD poisoned words behind it."""

    def __init__(self, dev, graph, threshold, floor, capacity=None):
        lib = _native.lib()
        edges, counts, sums, sizes = graph
        self.host = (np.array(edges, np.int32).reshape(-1, 2), np.array(counts, np.int64),
                     np.array(sums, np.uint64), np.array(sizes, np.int64))
        self.n_edges, self.k = len(self.host[1]), len(self.host[3]) - 1
        self.threshold, self.floor = float(threshold), int(floor)
        self.capacity = c = int(capacity or capacity_for(self.n_edges))
        self.inputs = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in self.host]
        self.need = lib.exaspim_region_graph_premerge_workspace_bytes(self.k, c)
        assert self.need >= 24 * c + 16 * (self.k + 1), _native.last_error()
        self.edges = torch.full((2 * c + GUARD,), -1234567, dtype=torch.int32, device=dev)
        self.counts = torch.full((c + GUARD,), -7654321, dtype=torch.int64, device=dev)
        self.sums = torch.full((c + GUARD,), -1111111, dtype=torch.int64, device=dev)
        self.sizes = torch.full((self.k + 1 + GUARD,), -2222222, dtype=torch.int64, device=dev)
        self.map = torch.full((self.k + 1 + GUARD,), -4444444, dtype=torch.int32, device=dev)
        self.state = torch.full((3 + GUARD,), -3333333, dtype=torch.int32, device=dev)
        self.ws = torch.full((self.need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)

    def args(self):
        e, c, s, z = self.inputs
        return [e.data_ptr(), c.data_ptr(), s.data_ptr(), z.data_ptr(), self.n_edges, self.k, self.threshold,
                self.floor, self.capacity, self.edges.data_ptr(), self.counts.data_ptr(), self.sums.data_ptr(),
                self.sizes.data_ptr(), self.map.data_ptr(), self.state.data_ptr(), self.ws.data_ptr(), self.need,
                None]

    def run(self, args=None):
        rc = _native.lib().exaspim_region_graph_premerge(*(self.args() if args is None else args))
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        c, k = self.capacity, self.k
        return bool((self.edges[2 * c:] == -1234567).all() and (self.counts[c:] == -7654321).all()
                    and (self.sums[c:] == -1111111).all() and (self.sizes[k + 1:] == -2222222).all()
                    and (self.map[k + 1:] == -4444444).all() and (self.state[3:] == -3333333).all()
                    and (self.ws[self.need:] == 0xFF).all())

    def untouched(self):
        c, k = self.capacity, self.k
        return bool(self.guards_intact() and (self.edges[:2 * c] == -1234567).all()
                    and (self.counts[:c] == -7654321).all() and (self.sums[:c] == -1111111).all()
                    and (self.sizes[:k + 1] == -2222222).all() and (self.map[:k + 1] == -4444444).all()
                    and (self.state[:3] == -3333333).all() and (self.ws[:self.need] == 0xFF).all())

    def inputs_untouched(self):
        return all(np.array_equal(t.cpu().numpy(), a.view(np.int64) if a.dtype == np.uint64 else a)
                   for t, a in zip(self.inputs, self.host))

    def result(self):
        """(edges', counts', sums', sizes', map) with the list sorted by (lo, hi), and the overflow flag."""
        k2, e2, overflow = (int(v) for v in self.state[:3].cpu())
        assert 0 <= e2 <= self.capacity and 0 <= k2 <= self.k
        edges = self.edges[:2 * e2].cpu().numpy().reshape(-1, 2)
        counts = self.counts[:e2].cpu().numpy()
        sums = self.sums[:e2].cpu().numpy().view(np.uint64)
        order = np.lexsort((edges[:, 1], edges[:, 0]))
        sizes = self.sizes[:self.k + 1].cpu().numpy()
        assert (sizes[k2 + 1:] == 0).all()   # the entries beyond K' are zeroed
        return (edges[order], counts[order], sums[order], sizes[:k2 + 1], self.map[:self.k + 1].cpu().numpy()), overflow


NAMES = ("edges", "counts", "sums", "sizes", "map")


def assert_same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


def check(dev, graph, threshold, floor, capacity=None):
    """One round on the device against the oracle; returns the oracle's (graph', map, depth)."""
    want = premerge_ref.one_round(*graph, threshold, floor)
    call = Call(dev, graph, threshold, floor, capacity)
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact() and call.inputs_untouched()
    got, overflow = call.result()
    assert overflow == 0
    assert_same(got, want[:5])
    return want


# ---- 1. random tie-heavy graphs, fragment counts around the scan's block ---------------------------
@pytest.mark.parametrize("k", [1, 2, 2047, 2048, 2049, 4097])
def test_random_tie_heavy_graphs_around_the_scan_block(dev, k):
    merged = False
    for seed, (levels, threshold, floor) in enumerate([(2, 0.6, 20), (4, 0.9, 10), (8, 0.3, 1000), (2, 1.5, 20)]):
        graph = premerge_ref.random_graph(100 * k + seed, k, 2 * k, levels)
        want = check(dev, graph, threshold, floor)
        merged |= len(want[3]) - 1 < k
    assert merged or k <= 2
    # the identity: floors 0, 1 (no fragment is empty) and a negative one
    for floor in (0, 1, -7):
        want = check(dev, graph, 0.9, floor)
        np.testing.assert_array_equal(want[4], np.arange(k + 1))
        assert_same(want[:4], graph)


# ---- 2. chains as long as the graph -------------------------------------------------------------
def line_graph(k, means):
    edges = np.array([(f, f + 1) for f in range(1, k)], np.int32)
    counts = np.full(k - 1, 3, np.int64)
    return edges, counts, (3 * np.asarray(means)).astype(np.uint64), np.full(k + 1, 2, np.int64)


@pytest.mark.parametrize("direction", ["rising", "falling"])
def test_a_line_of_5000_tiny_fragments_is_one_chain(dev, direction):
    k = 5000
    means = 1000 + np.arange(1, k) if direction == "rising" else 9000 - np.arange(1, k)
    *_, sizes2, mapping, depth = check(dev, line_graph(k, means), 1.5, 5)
    # rising: 1 -> 2 -> ... -> k - 1 <- k; falling: k -> ... -> 2 -> 1; the last two choose each other
    assert depth == (k - 2 if direction == "rising" else k - 1)
    assert len(sizes2) == 2 and sizes2[1] == 2 * k and (mapping[1:] == 1).all()


# ---- 3. all contention on one word ----------------------------------------------------------------
def test_3000_leaves_around_one_hub(dev):
    n = 3000
    edges = np.array([(1, f) for f in range(2, n + 2)], np.int32)
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 5, n).astype(np.int64)
    sums = (counts * (ONE - 5)).astype(np.uint64)
    sizes = np.concatenate([[17, 100000], rng.integers(1, 9, n)]).astype(np.int64)
    e2, _, _, sizes2, mapping, _ = check(dev, (edges, counts, sums, sizes), 0.9, 10)
    assert len(e2) == 0 and len(sizes2) == 2 and sizes2[1] == sizes[1:].sum() and (mapping[1:] == 1).all()


def test_two_hubs_sharing_3000_leaves(dev):
    n = 3000
    # the leaves prefer hub 1 or hub 2 by their means; the hubs are large, so every contracted edge is (1, 2)
    edges = np.array([(h, f) for f in range(3, n + 3) for h in (1, 2)], np.int32)
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 5, 2 * n).astype(np.int64)
    sums = (counts * rng.integers(ONE // 2, ONE, 2 * n)).astype(np.uint64)
    sizes = np.concatenate([[0, 50000, 60000], rng.integers(1, 9, n)]).astype(np.int64)
    e2, c2, s2, sizes2, mapping, _ = check(dev, (edges, counts, sums, sizes), 0.9, 10)
    assert e2.tolist() == [[1, 2]] and len(sizes2) == 3 and set(mapping[3:]) == {1, 2}
    assert c2[0] == counts.sum() - counts[(mapping[edges[:, 1]] == edges[:, 0])].sum()


# ---- 4. ties ---------------------------------------------------------------------------------------
def test_all_means_equal_on_a_grid(dev):
    h, w = 37, 41
    ids = np.arange(1, h * w + 1).reshape(h, w)
    pairs = np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1),
                            np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1)])
    edges = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int32)
    counts = np.random.default_rng(5).integers(1, 6, len(edges)).astype(np.int64)
    sums = (counts * (ONE // 2)).astype(np.uint64)   # every mean the same, whatever the count
    sizes = np.random.default_rng(6).choice([3, 50], h * w + 1).astype(np.int64)
    sizes[1] = sizes[2] = 3   # 1 and 2 choose each other; so does every tiny pair below a row of large ones
    *_, sizes2, mapping, _ = check(dev, (edges, counts, sums, sizes), 0.9, 4)
    assert 1 < len(sizes2) - 1 < h * w and mapping[2] == 1


def test_the_merge_bound_is_strict(dev):
    threshold = 0.75
    m, merge_all = premerge_ref.merge_bound(threshold)
    assert m == ONE // 4 and not merge_all
    edges = np.array([(1, 2), (2, 3), (3, 4)], np.int32)
    counts = np.array([7, 5, 3], np.int64)
    sizes = np.array([9, 1, 1, 1, 1], np.int64)
    at_the_bound = (edges, counts, (counts * m).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, at_the_bound, threshold, 10)[4], np.arange(5))
    above = (edges, counts, (counts * m + np.array([0, 1, 0])).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, above, threshold, 10)[4], [0, 1, 2, 2, 3])


def test_thresholds_above_one_merge_everything_and_zero_merges_nothing(dev):
    edges, counts, sums, sizes = premerge_ref.random_graph(8, 300, 500, 4)
    sums = sums.copy()
    sums[::3] = 0   # merge_all takes an edge of sum 0 as well
    want = check(dev, (edges, counts, sums, sizes), 1.5, 1000)
    assert len(want[3]) - 1 < 300
    # every fragment with an edge has merged: what is left has no edge at all
    assert len(premerge_ref.rounds(edges, counts, sums, sizes, 1.5, 10 ** 6, limit=20)[0][0]) == 0
    # T = 0 gives m = 2^24: no sum exceeds count * 2^24
    full = (counts.astype(np.uint64) << np.uint64(24))
    np.testing.assert_array_equal(check(dev, (edges, counts, full, sizes), 0.0, 1000)[4], np.arange(301))


def test_a_fragment_of_size_zero_is_tiny_at_floor_one(dev):
    edges = np.array([(1, 2), (2, 3), (3, 4)], np.int32)
    counts = np.array([2, 2, 2], np.int64)
    sums = np.array([2 * ONE - 9, 2 * ONE - 4, 2 * ONE - 2], np.uint64)
    sizes = np.array([5, 4, 0, 6, 0], np.int64)
    want = check(dev, (edges, counts, sums, sizes), 0.9, 1)
    np.testing.assert_array_equal(want[4], [0, 1, 2, 2, 2])   # 2 -> 3 and 4 -> 3
    np.testing.assert_array_equal(want[3], [5, 4, 6])


def test_ends_that_are_no_fragments_never_become_addresses(dev):
    edges, counts, sums, sizes = premerge_ref.random_graph(9, 50, 120, 2)
    bad = np.array([(0, 5), (3, 51), (-4, 7), (9, 9), (2147483647, 1), (6, -2147483648)], np.int32)
    dirty = (np.concatenate([edges, bad]), np.concatenate([counts, np.full(6, 3, np.int64)]),
             np.concatenate([sums, np.full(6, 3 * ONE, np.uint64)]), sizes)
    call = Call(dev, dirty, 0.9, 20)
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact() and call.inputs_untouched()
    got, overflow = call.result()
    assert overflow == 0
    assert_same(got, premerge_ref.one_round(edges, counts, sums, sizes, 0.9, 20)[:5])


# ---- 5. the call itself ---------------------------------------------------------------------------
def test_two_runs_are_identical_and_inputs_stay(dev):
    graph = premerge_ref.random_graph(21, 3000, 7000, 2)
    first = Call(dev, graph, 0.6, 20)
    assert first.run() == 0 and first.run() == 0   # the second run starts from the first one's leftovers
    second = Call(dev, graph, 0.6, 20)
    assert second.run() == 0
    assert first.guards_intact() and second.guards_intact() and first.inputs_untouched()
    a, b = first.result(), second.result()
    assert a[1] == b[1] == 0
    assert_same(a[0], b[0])
    assert torch.equal(first.state[:3], second.state[:3]) and torch.equal(first.map, second.map)
    assert torch.equal(first.sizes, second.sizes)


def test_a_table_that_is_too_small_raises_the_flag(dev):
    graph = premerge_ref.random_graph(22, 400, 900, 4)
    call = Call(dev, graph, 0.9, 0, capacity=64)   # the identity keeps every edge: far more than 64
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact()
    k2, _, overflow = (int(v) for v in call.state[:3].cpu())
    assert overflow == 1 and k2 == 400
    np.testing.assert_array_equal(call.map[:401].cpu().numpy(), np.arange(401))
    with pytest.raises(RuntimeError, match="edge_capacity"):
        inference.premerge_region_graph(*graph, 0.9, 0, edge_capacity=64)


def test_every_refusal_leaves_every_buffer_alone(dev):
    graph = premerge_ref.random_graph(23, 30, 60, 2)
    call = Call(dev, graph, 0.9, 10)
    good = call.args()

    def rc(index, value):
        args = list(good)
        args[index] = value
        return call.run(args)

    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15):
        assert rc(i, None) == -1 and "NULL" in _native.last_error(), i
    assert rc(4, -1) == -1 and rc(4, 1 << 31) == -1 and rc(5, -1) == -1
    assert rc(6, float("nan")) == -1 and "NaN" in _native.last_error()
    for capacity in (0, -8, call.capacity - 1, 3 * call.capacity, 1 << 31):
        assert rc(8, capacity) == -1 and "edge_capacity" in _native.last_error(), capacity
    for i, off in ((0, 2), (9, 2), (13, 2), (14, 2), (1, 4), (2, 4), (3, 4), (10, 4), (11, 4), (12, 4), (15, 8)):
        assert rc(i, good[i] + off) == -1 and "misaligned" in _native.last_error(), i
    assert rc(16, call.need - 1) == -3 and "workspace" in _native.last_error()
    assert rc(16, 0) == -3
    assert call.untouched() and call.inputs_untouched()
    assert call.run() == 0 and call.guards_intact()
    # an empty edge list may be NULL
    lonely = Call(dev, (np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint64),
                        np.array([4, 1, 2], np.int64)), 0.9, 10, capacity=1)
    args = lonely.args()
    args[0] = args[1] = args[2] = None
    assert lonely.run(args) == 0 and lonely.guards_intact()
    got, overflow = lonely.result()
    assert overflow == 0 and got[4].tolist() == [0, 1, 2] and got[3].tolist() == [4, 1, 2] and len(got[0]) == 0


# ---- 6. the Python entry points --------------------------------------------------------------------
def test_premerge_region_graph_runs_rounds_on_host_and_device_arrays(dev):
    graph = premerge_ref.random_graph(31, 2500, 6000, 4)
    want_graph, want_map, want_history = premerge_ref.rounds(*graph, 0.9, 20, limit=4)
    assert len(want_history) >= 2 and want_history[0] < 2500
    got = inference.premerge_region_graph(*graph, 0.9, 20)
    assert_same(got[:5], want_graph + (want_map,))
    assert got[5] == want_history
    on_device = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in graph]
    again = inference.premerge_region_graph(*on_device, 0.9, 20, rounds=4, edge_capacity=1 << 14)
    assert_same(again[:5], got[:5])
    assert again[5] == got[5]
    for t, a in zip(on_device, graph):
        np.testing.assert_array_equal(t.cpu().numpy(), a.view(np.int64) if a.dtype == np.uint64 else a)
    one = inference.premerge_region_graph(*graph, 0.9, 20, rounds=1)
    assert_same(one[:5], premerge_ref.one_round(*graph, 0.9, 20)[:5])
    assert one[5] == want_history[:1]


# ---- 7. wide operands: the high words of the 128-bit comparisons decide ----------------------------
@pytest.mark.parametrize("k", [1, 2, 2047, 2048, 2049, 4097, 3000])
def test_wide_near_ties_around_the_scan_block(dev, k):
    """Counts up to 2^27, sum = count * level + {-1, 0, 1}: the cross products need up to 2^78, the
    contracted counts and sums up to 2^39 and 2^63."""
    graph = region_graph_ref.wide_graph(500 + k, k, 3 * k if k == 3000 else 2 * k, 5, 1 << 27)
    edges, counts, sums, _ = graph
    assert sum(counts.tolist()) <= 1 << 39
    if k >= 2047:
        products = [s * c for s, c in zip(sums[:-1].tolist(), counts[1:].tolist())]
        assert 2 * sum(p >= 1 << 64 for p in products) >= len(products)
    merged = False
    for threshold, floor in ((0.3, 20), (0.55, 10), (0.8, 1000)):
        want = check(dev, graph, threshold, floor)
        merged |= len(want[3]) - 1 < k
        assert k < 2047 or int(want[2].max()) > 1 << 50      # sums' far beyond 32 bits
        want_graph, want_map, want_history = premerge_ref.rounds(*graph, threshold, floor, limit=4)
        got = inference.premerge_region_graph(*graph, threshold, floor)
        assert_same(got[:5], want_graph + (want_map,))
        assert got[5] == want_history
    assert k <= 2 or merged


def wide_hub(tiny):
    """
    Fragment 2 is a hub of 3000 leaves (3 .. 3002), which all touch fragment 1 as well. The hub's contacts
    have counts up to 2^27 and means a hair around 15/16 or 31/32, all above the bound of T = 0.1; the
    contacts with fragment 1 have means around 7/8, below it. tiny="hub": the 3000 edges bid for the hub's
    one word. tiny="leaves": every leaf joins the hub, and their contacts with 1 pool into one.
    """
    n = 3000
    rng = np.random.default_rng(12)
    leaves = np.arange(3, n + 3)
    edges = np.array([(end, f) for end in (1, 2) for f in leaves], np.int32)
    counts = rng.integers(1, (1 << 27) + 1, 2 * n).astype(np.int64)
    level = np.concatenate([np.full(n, 7 * ONE // 8), rng.choice([15 * ONE // 16, 31 * ONE // 32], n)])
    sums = (counts * level + rng.integers(-1, 2, 2 * n)).astype(np.uint64)
    if tiny == "hub":
        sizes = np.concatenate([[0, 10 ** 6, 1], np.full(n, 1000)]).astype(np.int64)
    else:
        sizes = np.concatenate([[0, 10 ** 6, 10 ** 5], rng.integers(1, 9, n)]).astype(np.int64)
    assert sum(counts.tolist()) <= 1 << 39
    return edges, counts, sums, sizes


@pytest.mark.parametrize("tiny", ["hub", "leaves"])
def test_a_hub_of_3000_wide_near_tied_contacts(dev, tiny):
    graph = wide_hub(tiny)
    edges, counts, sums, sizes = graph
    m, _ = premerge_ref.merge_bound(0.1)
    hub_edges = edges[:, 0] == 2
    assert all(s > m * c for c, s in zip(counts[hub_edges].tolist(), sums[hub_edges].tolist()))
    assert not any(s > m * c for c, s in zip(counts[~hub_edges].tolist(), sums[~hub_edges].tolist()))
    e2, c2, s2, sizes2, mapping, _ = check(dev, graph, 0.1, 10)
    if tiny == "hub":
        # the hub joins one leaf: the exact maximum of 3000 means that agree to some 2^-27
        best = max(np.flatnonzero(hub_edges).tolist(),
                   key=lambda e: (Fraction(int(sums[e]), int(counts[e])), -int(edges[e, 1])))
        assert len(sizes2) - 1 == 3001 and mapping[2] == mapping[edges[best, 1]] == 2
        products = [s * c for s, c in zip(sums[hub_edges][:-1].tolist(), counts[hub_edges][1:].tolist())]
        assert 2 * sum(p >= 1 << 64 for p in products) >= len(products)      # the high words decide
    else:
        assert len(sizes2) - 1 == 2 and e2.tolist() == [[1, 2]]
        assert int(c2[0]) == sum(counts[~hub_edges].tolist()) > 1 << 37
        assert int(s2[0]) == sum(sums[~hub_edges].tolist()) > 1 << 61
    # two runs, the second on the first one's leftovers, and a fresh call
    first, second = Call(dev, graph, 0.1, 10), Call(dev, graph, 0.1, 10)
    assert first.run() == 0 and first.run() == 0 and second.run() == 0
    assert first.guards_intact() and second.guards_intact() and first.inputs_untouched()
    a, b = first.result(), second.result()
    assert a[1] == b[1] == 0
    assert_same(a[0], b[0])
    assert_same(a[0], (e2, c2, s2, sizes2, mapping))
    assert torch.equal(first.state[:3], second.state[:3]) and torch.equal(first.map, second.map)


def test_a_total_count_above_2_39_is_refused_before_the_first_round(dev):
    edges = np.array([(1, f) for f in range(2, 35)], np.int32)
    counts = np.full(33, 1 << 34, np.int64)
    sums = (counts * (ONE - 3)).astype(np.uint64)
    sizes = np.full(35, 5, np.int64)
    total = 33 << 34
    with pytest.raises(ValueError, match=str(total)):
        inference.premerge_region_graph(edges, counts, sums, sizes, 0.9, 10)
    on_device = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
                 for a in (edges, counts, sums, sizes)]
    with pytest.raises(ValueError, match=str(total)):
        inference.premerge_region_graph(*on_device, 0.9, 10)
    # two of the contacts halved: 2^39 exactly, which runs
    counts[-1], counts[-2] = 1 << 33, 1 << 33
    sums = (counts * (ONE - 3)).astype(np.uint64)
    assert sum(counts.tolist()) == 1 << 39
    on_device = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
                 for a in (edges, counts, sums, sizes)]
    got = inference.premerge_region_graph(*on_device, 0.9, 10, rounds=1)
    assert_same(got[:5], premerge_ref.one_round(edges, counts, sums, sizes, 0.9, 10)[:5])


THRESHOLDS = [0.6, 0.8, 0.9]
_CHAIN = {}


def oracle_chain(kind, shape, dtype=np.float32):
    """The oracle's labels and round history for floor 25, computed once per case."""
    key = (kind, shape, np.dtype(dtype).name)
    if key not in _CHAIN:
        aff = watershed_ref.random_affinities(kind, shape).astype(dtype)
        fragments, k = watershed_ref.fragments(aff)
        graph = region_graph_ref.region_graph(fragments, aff, k)
        reduced, composed, history = premerge_ref.rounds(*graph, THRESHOLDS[-1], 25, limit=4)
        table, _ = region_graph_ref.agglomerate(*reduced, THRESHOLDS[-1], 100)
        labels = table[composed][fragments].astype(np.int32)
        labels.setflags(write=False)
        _CHAIN[key] = (aff, labels, k, history)
    return _CHAIN[key]


@pytest.mark.parametrize("shape", [(9, 9, 33), (17, 17, 65)])
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_end_to_end_equals_the_oracle_chain(dev, kind, shape):
    aff, want, k, history = oracle_chain(kind, shape)
    got = inference.agglomerate_affinities(aff, THRESHOLDS, 100, fragments="watershed", premerge_size=25)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    if (kind, shape) == ("uniform", (17, 17, 65)):
        # a third round that still merges, a fourth that does not, and more than one fragment left
        assert k == 5118 and len(history) == 4 and history[2] < history[1] < history[0] < k
        assert history[3] == history[2] > 1
    on_device = inference.agglomerate_affinities(torch.from_numpy(np.array(aff)).to(dev), THRESHOLDS, 100,
                                                 fragments="watershed", premerge_size=25,
                                                 return_device_tensor=True)
    assert on_device.device.type == "cuda" and np.array_equal(on_device.cpu().numpy(), want)


def test_a_floor_of_one_gives_the_labels_of_no_floor(dev):
    for kind in ("uniform", "smooth"):
        aff = np.array(watershed_ref.random_affinities(kind, (17, 17, 65)))
        plain =inference.agglomerate_affinities(aff, THRESHOLDS, 30, fragments="watershed")
        floor1 = inference.agglomerate_affinities(aff, THRESHOLDS, 30, fragments="watershed", premerge_size=1,
                                                  premerge_rounds=2)
        np.testing.assert_array_equal(floor1, plain)
        floor25 = inference.agglomerate_affinities(aff, THRESHOLDS, 30, fragments="watershed", premerge_size=25)
        assert plain.max() >= 1 and floor25.shape == plain.shape and floor25.max() >= 1


def test_float16_affinities(dev):
    aff, want, _, _ = oracle_chain("smooth", (9, 9, 33), np.float16)
    assert aff.dtype == np.float16
    got = inference.agglomerate_affinities(aff, THRESHOLDS, 100, fragments="watershed", premerge_size=25)
    np.testing.assert_array_equal(got, want)


def test_components_as_fragments_with_a_floor(dev):
    import components_ref

    aff = np.array(watershed_ref.random_affinities("uniform", (9, 9, 33)))
    fragments, k = components_ref.components(aff, 0.75, 0)
    graph = region_graph_ref.region_graph(fragments, aff, k)
    reduced, composed, history = premerge_ref.rounds(*graph, 0.5, 6, limit=4)
    assert history[0] < k
    table, _ = region_graph_ref.agglomerate(*reduced, 0.5, 10)
    got = inference.agglomerate_affinities(aff, [0.5], 10, fragment_threshold=0.75, premerge_size=6)
    np.testing.assert_array_equal(got, table[composed][fragments])


@pytest.mark.parametrize("threshold", [0.6, 0.7])
def test_end_to_end_at_sixteen_thousand_fragments(dev, threshold):
    """(33, 65, 129) watershed fragments, floor 25: premerge_ref.rounds, then the heap oracle (the naive one
    would take hours here)."""
    aff, fragments, k, graph = region_graph_ref.fragment_volume("watershed")
    aff = np.array(aff)                         # the shared one is read-only
    reduced, composed, history = premerge_ref.rounds(*graph, threshold, 25, limit=4)
    table, s = region_graph_ref.agglomerate_fast(*reduced, threshold, 0)
    assert k >= 10000 and history[0] < k and 1 < s < history[-1]
    got = inference.agglomerate_affinities(aff, [threshold], 0, fragments="watershed", aff_threshold_low=0.3,
                                           aff_threshold_high=0.7, premerge_size=25)
    np.testing.assert_array_equal(got, table[composed][fragments])
