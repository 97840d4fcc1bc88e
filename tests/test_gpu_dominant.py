"""
exaspim_region_graph_contract_dominant, inference.contract_dominant_edges and
agglomerate_affinities(device_merge_rounds=...) on the GPU (-m gpu), array for array against the
Python-integer oracle of tests/dominant_ref.py: the edge list after sorting by (lo, hi), map, sizes', K'
and E' exact; end to end the labels are those of the same call with device_merge_rounds=0, bit for bit.

The graphs sit where the kernels can go wrong: fragment counts around the scan's block of 2048, thousands
of bids for one best[] word, ties that must hold an edge back (equal means of different count and sum,
means that differ only beyond the low 64 bits of the cross product), the merge bound hit exactly, rows
that are no edges. Every direct call runs with 0xFF in every output buffer, guard words behind each and
a workspace pre-filled with 0xFF.
"""

import numpy as np
import pytest
import torch

import dominant_ref
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


def to_device(graph, dev):
    return [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in graph]


class Call:
    """One exaspim_region_graph_contract_dominant call: every output is 0xFF bytes with GUARD more behind it."""

    def __init__(self, dev, graph, threshold, capacity=None):
        lib = _native.lib()
        edges, counts, sums, sizes = graph
        self.host = (np.array(edges, np.int32).reshape(-1, 2), np.array(counts, np.int64),
                     np.array(sums, np.uint64), np.array(sizes, np.int64))
        self.n_edges, self.k = len(self.host[1]), len(self.host[3]) - 1
        self.threshold = float(threshold)
        self.capacity = c = int(capacity or capacity_for(self.n_edges))
        self.inputs = to_device(self.host, dev)
        self.need = lib.exaspim_region_graph_contract_dominant_workspace_bytes(self.k, c)
        assert self.need >= 24 * c + 12 * (self.k + 1), _native.last_error()
        self.edges = torch.full((2 * c + GUARD,), -1, dtype=torch.int32, device=dev)
        self.counts = torch.full((c + GUARD,), -1, dtype=torch.int64, device=dev)
        self.sums = torch.full((c + GUARD,), -1, dtype=torch.int64, device=dev)
        self.sizes = torch.full((self.k + 1 + GUARD,), -1, dtype=torch.int64, device=dev)
        self.map = torch.full((self.k + 1 + GUARD,), -1, dtype=torch.int32, device=dev)
        self.state = torch.full((3 + GUARD,), -1, dtype=torch.int32, device=dev)
        self.ws = torch.full((self.need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)

    def args(self):
        e, c, s, z = self.inputs
        return [e.data_ptr(), c.data_ptr(), s.data_ptr(), z.data_ptr(), self.n_edges, self.k, self.threshold,
                self.capacity, self.edges.data_ptr(), self.counts.data_ptr(), self.sums.data_ptr(),
                self.sizes.data_ptr(), self.map.data_ptr(), self.state.data_ptr(), self.ws.data_ptr(), self.need,
                None]

    def run(self, args=None):
        rc = _native.lib().exaspim_region_graph_contract_dominant(*(self.args() if args is None else args))
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        c, k = self.capacity, self.k
        return bool((self.edges[2 * c:] == -1).all() and (self.counts[c:] == -1).all()
                    and (self.sums[c:] == -1).all() and (self.sizes[k + 1:] == -1).all()
                    and (self.map[k + 1:] == -1).all() and (self.state[3:] == -1).all()
                    and (self.ws[self.need:] == 0xFF).all())

    def untouched(self):
        return bool(all((t == -1).all() for t in (self.edges, self.counts, self.sums, self.sizes, self.map,
                                                   self.state)) and (self.ws == 0xFF).all())

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


def check(dev, graph, threshold, capacity=None, want=None):
    """One round on the device against the oracle; returns the oracle's (graph', map)."""
    if want is None:
        want = dominant_ref.one_round(*graph, threshold)
    call = Call(dev, graph, threshold, capacity)
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact() and call.inputs_untouched()
    got, overflow = call.result()
    assert overflow == 0
    assert_same(got, want)
    return want


# ---- 1. random tie-heavy graphs, fragment counts around the scan's block ---------------------------
@pytest.mark.parametrize("k", [1, 2, 2047, 2048, 2049, 4097])
def test_tie_heavy_random_graphs_around_the_scan_block(dev, k):
    contracted = held_back = False
    for seed, threshold in enumerate([0.5, 0.6, 0.75, 0.9, 1.5]):
        graph = dominant_ref.tie_heavy_graph(100 * k + seed, k, 2 * k)
        want = check(dev, graph, threshold)
        contracted |= len(want[3]) - 1 < k
        held_back |= len(want[0]) > 0
    assert (contracted and held_back) or k <= 2
    if k == 2:      # one edge between the two fragments: it dominates at both, and nothing is left
        graph = (np.array([(1, 2)], np.int32), np.array([2], np.int64), np.array([ONE], np.uint64),
                 np.array([5, 3, 4], np.int64))
        want = check(dev, graph, 0.9)
        assert want[4].tolist() == [0, 1, 1] and want[3].tolist() == [5, 7] and len(want[0]) == 0


# ---- 2. lines --------------------------------------------------------------------------------------
def line_graph(k, means):
    edges = np.array([(f, f + 1) for f in range(1, k)], np.int32)
    counts = np.full(k - 1, 3, np.int64)
    return edges, counts, (3 * np.asarray(means)).astype(np.uint64), np.full(k + 1, 2, np.int64)


@pytest.mark.parametrize("direction", ["rising", "falling"])
def test_a_line_of_5000_fragments_contracts_exactly_one_pair(dev, direction):
    k = 5000
    means = 1000 + np.arange(1, k) if direction == "rising" else 9000 - np.arange(1, k)
    *_, sizes2, mapping = check(dev, line_graph(k, means), 1.5)
    assert len(sizes2) - 1 == k - 1
    pair = (k - 1, k) if direction == "rising" else (1, 2)
    assert mapping[pair[0]] == mapping[pair[1]] and sizes2[mapping[pair[0]]] == 4
    assert np.bincount(mapping[1:]).max() == 2 and (np.bincount(mapping[1:]) == 2).sum() == 1


def test_a_line_of_alternating_means_halves(dev):
    k = 5000
    means = np.where(np.arange(1, k) % 2 == 1, 9000 + np.arange(1, k), 100 + np.arange(1, k))
    *_, sizes2, mapping = check(dev, line_graph(k, means), 1.5)
    assert len(sizes2) - 1 == k // 2 and (sizes2[1:] == 4).all()
    np.testing.assert_array_equal(mapping[1:], (np.arange(1, k + 1) + 1) // 2)


# ---- 3. ties hold an edge back ---------------------------------------------------------------------
def test_all_means_equal_on_a_grid_contract_nothing(dev):
    h, w = 37, 41
    ids = np.arange(1, h * w + 1).reshape(h, w)
    pairs = np.concatenate([np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1),
                            np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1)])
    edges = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))].astype(np.int32)
    counts = np.random.default_rng(5).integers(1, 6, len(edges)).astype(np.int64)
    sums = (counts * (ONE // 2)).astype(np.uint64)   # every mean the same, whatever the count
    sizes = np.random.default_rng(6).integers(1, 50, h * w + 1).astype(np.int64)
    graph = (edges, counts, sums, sizes)
    want = check(dev, graph, 0.9)
    np.testing.assert_array_equal(want[4], np.arange(h * w + 1))
    assert_same(want[:4], graph)


def hub_graph(n, tie_the_top_two):
    """Fragment 1 with n leaves of distinct means, in a shuffled order; optionally the best two tied with
    different (count, sum)."""
    rng = np.random.default_rng(3)
    edges = np.array([(1, f) for f in range(2, n + 2)], np.int32)
    counts = rng.integers(1, 5, n).astype(np.int64)
    level = rng.permutation(n) + ONE // 2           # distinct means
    sums = counts * level
    best, second = int(np.argmax(level)), int(np.argsort(level)[-2])
    if tie_the_top_two:
        counts[best], counts[second] = 3, 4
        sums[best], sums[second] = 3 * (ONE - 7), 4 * (ONE - 7)
    sizes = rng.integers(1, 9, n + 2).astype(np.int64)
    return (edges, counts, sums.astype(np.uint64), sizes), best


def test_a_hub_of_3000_leaves_contracts_only_its_best_leaf(dev):
    graph, best = hub_graph(3000, False)
    e2, _, _, sizes2, mapping = check(dev, graph, 0.9)
    assert len(sizes2) - 1 == 3000 and mapping[best + 2] == mapping[1] == 1 and len(e2) == 2999
    assert sizes2[1] == graph[3][1] + graph[3][best + 2]


def test_a_hub_whose_top_two_leaves_tie_contracts_nothing(dev):
    graph, _ = hub_graph(3000, True)
    want = check(dev, graph, 0.9)
    np.testing.assert_array_equal(want[4], np.arange(3002))
    assert_same(want[:4], graph)


def test_two_hubs_sharing_3000_leaves(dev):
    n = 3000
    edges = np.array([(h, f) for f in range(3, n + 3) for h in (1, 2)], np.int32)
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 5, 2 * n).astype(np.int64)
    sums = (counts * (rng.permutation(2 * n) + ONE // 2)).astype(np.uint64)      # 6000 distinct means
    sizes = rng.integers(1, 9, n + 3).astype(np.int64)
    e2, _, _, sizes2, mapping = check(dev, (edges, counts, sums, sizes), 0.9)
    # each hub pairs with its best leaf, unless both want the same one: then only the better edge goes
    assert len(sizes2) - 1 in (n, n + 1) and np.bincount(mapping[1:]).max() == 2
    assert len(e2) < 2 * n


# ---- 4. wide operands: strictness in 128 bits -------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 2047, 2048, 2049, 4097])
def test_wide_near_ties_around_the_scan_block(dev, k):
    """Counts up to 2^34 (2^27 where the total would pass 2^39), sum = count * level + {-1, 0, 1}: equal
    levels give means that differ by less than 2^-27, and cross products up to 2^92."""
    count_max = 1 << 34 if k <= 2 else 1 << 27
    graph = region_graph_ref.wide_graph(900 + k, k, 2 * k, 5, count_max)
    edges, counts, sums, _ = graph
    assert sum(counts.tolist()) <= 1 << 39
    if k >= 2047:
        products = [s * c for s, c in zip(sums[:-1].tolist(), counts[1:].tolist())]
        assert 2 * sum(p >= 1 << 64 for p in products) >= len(products)
    contracted = False
    for threshold in (0.3, 0.55, 0.8):
        want = check(dev, graph, threshold)
        contracted |= len(want[3]) - 1 < k
    assert k <= 2 or contracted


def wide_hub(kind):
    """
    Fragment 1 with 3000 leaves whose counts are near 2^34 (the first 30) or below 2^20, all of mean a hair
    around 15/16. kind="low word": the best two means have cross products that agree in their high 64 bits
    and differ in the low ones (count 2^34 - 1 and 2^34 - 3, the same level, sums off by one); the hub
    contracts its best leaf. kind="equal": the best two means are exactly equal with different (count,
    sum), counts 2^34 and 2^33: the hub contracts nothing.
    """
    n = 3000
    rng = np.random.default_rng(12)
    level = 15 * ONE // 16
    counts = np.concatenate([rng.integers((1 << 34) - 4096, 1 << 34, 28), rng.integers(1, 1 << 20, n - 28)])
    sums = counts * level - rng.integers(2, 50, n)      # every mean below the level
    if kind == "low word":
        top = np.array([(1 << 34) - 1, (1 << 34) - 3])
        top_sums = top * level + np.array([1, 0])       # level + 1 / (2^34 - 1) against the level itself
    else:
        top = np.array([1 << 34, 1 << 33])
        top_sums = top * level + np.array([2, 1])       # level + 2^-33, twice
    where = [1717, 404]                                 # the two rows that matter, far apart in the list
    counts, sums = counts.tolist(), sums.tolist()
    for i, c, s in zip(where, top.tolist(), top_sums.tolist()):
        counts[i], sums[i] = c, s
    assert sum(counts) <= 1 << 39 and all(0 <= s <= c * ONE for c, s in zip(counts, sums))
    edges = np.array([(1, f) for f in range(2, n + 2)], np.int32)
    return (edges, np.array(counts, np.int64), np.array(sums, np.uint64), rng.integers(1, 9, n + 2).astype(np.int64)), where


@pytest.mark.parametrize("kind", ["low word", "equal"])
def test_a_hub_of_wide_near_ties(dev, kind):
    graph, (a, b) = wide_hub(kind)
    _, counts, sums, _ = graph
    left, right = int(sums[a]) * int(counts[b]), int(sums[b]) * int(counts[a])
    assert left >= 1 << 64
    if kind == "low word":
        assert left > right and left >> 64 == right >> 64      # only the low words tell them apart
    else:
        assert left == right and (int(counts[a]), int(sums[a])) != (int(counts[b]), int(sums[b]))
    *_, sizes2, mapping = check(dev, graph, 0.1)
    if kind == "low word":
        assert len(sizes2) - 1 == 3000 and mapping[a + 2] == mapping[1] == 1
    else:
        np.testing.assert_array_equal(mapping, np.arange(3002))


# ---- 5. the merge bound ------------------------------------------------------------------------------
def test_the_merge_bound_is_strict_and_a_row_at_the_bound_does_not_tie(dev):
    threshold = 0.75
    m, merge_all = premerge_ref.merge_bound(threshold)
    assert m == ONE // 4 and not merge_all
    edges = np.array([(1, 2), (2, 3), (3, 4)], np.int32)
    counts = np.array([7, 5, 3], np.int64)
    sizes = np.array([9, 1, 1, 1, 1], np.int64)
    at_the_bound = (edges, counts, (counts * m).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, at_the_bound, threshold)[4], np.arange(5))
    above = (edges, counts, (counts * m + np.array([0, 1, 0])).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, above, threshold)[4], [0, 1, 2, 2, 3])
    # 1-2 and 2-3 have the same mean, exactly the bound, and 3-4 is above it: were the rows at the bound
    # edges to be reckoned with, nothing could be said about 3; they are not, and 3-4 goes
    tie_below = (edges, counts, (counts * m + np.array([0, 0, 1])).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, tie_below, threshold)[4], [0, 1, 2, 3, 3])
    # a mergeable row that ties the best one does hold it back
    tie_above = (edges, counts, (counts * (m + 1)).astype(np.uint64), sizes)
    np.testing.assert_array_equal(check(dev, tie_above, threshold)[4], np.arange(5))


def test_thresholds_above_one_merge_everything_and_zero_merges_nothing(dev):
    edges, counts, sums, sizes = premerge_ref.random_graph(8, 300, 500, 4)
    sums = sums.copy()
    sums[::3] = 0   # merge_all takes an edge of sum 0 as well
    # a fragment whose only edges have sum 0 cannot contract (they tie) unless it has just one
    lonely = np.array([(301, 302)], np.int32)
    graph = (np.concatenate([edges, lonely]), np.append(counts, 4), np.append(sums, np.uint64(0)),
             np.append(sizes, [3, 5]).astype(np.int64))
    want = check(dev, graph, 1.5)
    assert len(want[3]) - 1 < 302 and want[4][301] == want[4][302]
    not_at_all = check(dev, graph, 1.0)      # m = 0: a sum of 0 is not above it
    assert not_at_all[4][301] != not_at_all[4][302]
    # T = 0 gives m = 2^24: no sum exceeds count * 2^24
    full = (counts.astype(np.uint64) << np.uint64(24))
    np.testing.assert_array_equal(check(dev, (edges, counts, full, sizes), 0.0)[4], np.arange(301))


# ---- 6. rows that are no edges ----------------------------------------------------------------------
def test_rows_that_are_no_edges_never_become_addresses_and_never_tie(dev):
    edges, counts, sums, sizes = dominant_ref.tie_heavy_graph(9, 50, 120)
    listed = set(map(tuple, edges.tolist()))
    empty = [(lo, lo + 1) for lo in range(1, 50) if (lo, lo + 1) not in listed][:2]      # count 0, ends that exist
    bad = np.array([(0, 5), (3, 51), (-4, 7), (9, 9), (2147483647, 1), (6, -2147483648)] + empty, np.int32)
    bad_counts = np.array([3, 3, 3, 3, 3, 3, 0, 0], np.int64)
    dirty = (np.concatenate([edges, bad]), np.concatenate([counts, bad_counts]),
             np.concatenate([sums, np.full(8, 3 * ONE, np.uint64)]), sizes)
    want = dominant_ref.one_round(edges, counts, sums, sizes, 0.9)
    assert len(want[3]) - 1 < 50
    assert_same(dominant_ref.one_round(*dirty, 0.9), want)      # the oracle skips them
    check(dev, dirty, 0.9, want=want)
    # a bad row of the largest mean at both ends of a dominant edge does not hold it back
    graph = (np.array([(1, 2), (1, 1), (2, 9), (1, 2)], np.int32), np.array([2, 1, 1, 0], np.int64),
             np.array([ONE, ONE, ONE, ONE], np.uint64), np.array([0, 4, 5], np.int64))
    got = check(dev, graph, 0.9)
    assert got[4].tolist() == [0, 1, 1] and got[3].tolist() == [0, 9]


# ---- 7. the call itself -------------------------------------------------------------------------------
def test_two_runs_are_identical_and_inputs_stay(dev):
    graph = dominant_ref.tie_heavy_graph(21, 3000, 7000)
    first = Call(dev, graph, 0.6)
    assert first.run() == 0 and first.run() == 0   # the second run starts from the first one's leftovers
    second = Call(dev, graph, 0.6)
    assert second.run() == 0
    assert first.guards_intact() and second.guards_intact() and first.inputs_untouched()
    a, b = first.result(), second.result()
    assert a[1] == b[1] == 0
    assert_same(a[0], b[0])
    assert_same(a[0], dominant_ref.one_round(*graph, 0.6))
    assert torch.equal(first.state[:3], second.state[:3]) and torch.equal(first.map, second.map)
    assert torch.equal(first.sizes, second.sizes)


def test_a_table_that_is_too_small_raises_the_flag(dev):
    graph = dominant_ref.tie_heavy_graph(22, 400, 900)
    want = dominant_ref.one_round(*graph, 0.9)
    assert len(want[0]) > 200
    call = Call(dev, graph, 0.9, capacity=64)
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact()
    k2, _, overflow = (int(v) for v in call.state[:3].cpu())
    assert overflow == 1 and k2 == len(want[3]) - 1
    np.testing.assert_array_equal(call.map[:401].cpu().numpy(), want[4])            # map and sizes' are intact
    np.testing.assert_array_equal(call.sizes[:k2 + 1].cpu().numpy(), want[3])
    with pytest.raises(RuntimeError, match="edge_capacity"):
        inference.contract_dominant_edges(*graph, 0.9, edge_capacity=64)


def test_every_refusal_leaves_every_buffer_alone(dev):
    graph = dominant_ref.tie_heavy_graph(23, 30, 60)
    call = Call(dev, graph, 0.9)
    good = call.args()

    def rc(index, value):
        args = list(good)
        args[index] = value
        return call.run(args)

    for i in (0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14):
        assert rc(i, None) == -1 and "NULL" in _native.last_error(), i
    assert rc(4, -1) == -1 and rc(4, 1 << 31) == -1 and rc(5, -1) == -1
    assert rc(6, float("nan")) == -1 and "NaN" in _native.last_error()
    for capacity in (0, -8, call.capacity - 1, 3 * call.capacity, 1 << 31):
        assert rc(7, capacity) == -1 and "edge_capacity" in _native.last_error(), capacity
    for i, off in ((0, 2), (8, 2), (12, 2), (13, 2), (1, 4), (2, 4), (3, 4), (9, 4), (10, 4), (11, 4), (14, 8)):
        assert rc(i, good[i] + off) == -1 and "misaligned" in _native.last_error(), i
    assert rc(15, call.need - 1) == -3 and "workspace" in _native.last_error()
    assert rc(15, 0) == -3
    assert call.untouched() and call.inputs_untouched()
    assert call.run() == 0 and call.guards_intact()
    # an empty edge list may be NULL
    lonely = Call(dev, (np.zeros((0, 2), np.int32), np.zeros(0, np.int64), np.zeros(0, np.uint64),
                        np.array([4, 1, 2], np.int64)), 0.9, capacity=1)
    args = lonely.args()
    args[0] = args[1] = args[2] = None
    assert lonely.run(args) == 0 and lonely.guards_intact()
    got, overflow = lonely.result()
    assert overflow == 0 and got[4].tolist() == [0, 1, 2] and got[3].tolist() == [4, 1, 2] and len(got[0]) == 0


def test_a_total_count_above_2_39_is_refused_before_the_first_round(dev):
    edges = np.array([(1, f) for f in range(2, 35)], np.int32)
    counts = np.full(33, 1 << 34, np.int64)
    sums = (counts * (ONE - 3) - np.arange(33)).astype(np.uint64)
    sizes = np.full(35, 5, np.int64)
    total = 33 << 34
    with pytest.raises(ValueError, match=str(total)):
        inference.contract_dominant_edges(edges, counts, sums, sizes, 0.9)
    with pytest.raises(ValueError, match=str(total)):
        inference.contract_dominant_edges(*to_device((edges, counts, sums, sizes), dev), 0.9)
    # two of the contacts halved: 2^39 exactly, which runs
    counts[-1], counts[-2] = 1 << 33, 1 << 33
    sums = (counts * (ONE - 3) - np.arange(33)).astype(np.uint64)
    assert sum(counts.tolist()) == 1 << 39
    got = inference.contract_dominant_edges(*to_device((edges, counts, sums, sizes), dev), 0.9, rounds=1)
    want = dominant_ref.one_round(edges, counts, sums, sizes, 0.9)
    assert len(want[3]) - 1 == 33
    assert_same(got[:5], want)


# ---- 8. the Python entry point ---------------------------------------------------------------------
def test_contract_dominant_edges_runs_rounds_on_host_and_device_arrays(dev):
    graph = region_graph_ref.mean_graph(31, 2500, 6000)
    want_graph, want_map, want_history = dominant_ref.rounds(*graph, 0.9)
    assert len(want_history) >= 3 and want_history[0] < 2500 * 7 // 8      # continuous means: rounds that pay
    got = inference.contract_dominant_edges(*graph, 0.9)
    assert_same(got[:5], want_graph + (want_map,))
    assert got[5] == want_history
    on_device = to_device(graph, dev)
    again = inference.contract_dominant_edges(*on_device, 0.9, rounds=64, edge_capacity=1 << 14)
    assert_same(again[:5], got[:5])
    assert again[5] == got[5]
    for t, a in zip(on_device, graph):
        np.testing.assert_array_equal(t.cpu().numpy(), a.view(np.int64) if a.dtype == np.uint64 else a)
    two = inference.contract_dominant_edges(*graph, 0.9, rounds=2)
    want_two = dominant_ref.rounds(*graph, 0.9, limit=2)
    assert_same(two[:5], want_two[0] + (want_two[1],))
    assert two[5] == want_history[:2]
    # the theorem, with the device's reduction: the host merger ends where it would have ended
    table, count = inference.agglomerate(*got[:4], [0.9], 30)
    want_table, want_count = inference.agglomerate(*graph, [0.9], 30)
    np.testing.assert_array_equal(table[got[4]], want_table)
    assert count == want_count
    # a tie-heavy graph through the rounds as well
    ties = dominant_ref.tie_heavy_graph(32, 2500, 6000)
    want_graph, want_map, want_history = dominant_ref.rounds(*ties, 0.6)
    got = inference.contract_dominant_edges(*ties, 0.6)
    assert_same(got[:5], want_graph + (want_map,))
    assert got[5] == want_history and want_history[0] < 2500


# ---- 9. end to end: the labels of device_merge_rounds=0, bit for bit ---------------------------------
def oracle_first_round(aff, kind, threshold, premerge_size=0, **how):
    """(K, K' after the first dominant round) by the oracles, after the pre-merge rounds if there are any."""
    if kind == "watershed":
        fragments, k = watershed_ref.fragments(aff, how.get("low", 0.1), how.get("high", 0.9999))
    else:
        import components_ref

        fragments, k = components_ref.components(aff, how["fragment_threshold"], 0)
    graph = region_graph_ref.region_graph(fragments, aff, k)
    if premerge_size:
        graph, _, history = premerge_ref.rounds(*graph, threshold, premerge_size, limit=4)
        k = history[-1]
    return k, len(dominant_ref.one_round(*graph, threshold)[3]) - 1


@pytest.mark.parametrize("shape", [(9, 9, 33), (17, 17, 65)])
@pytest.mark.parametrize("kind", ["uniform", "smooth"])
@pytest.mark.parametrize("fragments", ["watershed", "components"])
def test_end_to_end_equals_the_call_without_device_rounds(dev, fragments, kind, shape):
    aff = np.array(watershed_ref.random_affinities(kind, shape))
    # components: a cut just above the volume's percolation point, so that there are many of them
    cut = 0.75 if kind == "uniform" else 0.55
    how = dict(fragments=fragments) if fragments == "watershed" else dict(fragment_threshold=cut)
    for threshold in (0.6, 0.7):
        k, k2 = oracle_first_round(aff, fragments, threshold, fragment_threshold=cut)
        assert k2 < k, (k, k2)                                     # round one removes a fragment
        want = inference.agglomerate_affinities(aff, [threshold], 30, **how)
        assert want.max() >= 1
        for rounds in (1, 64):
            got = inference.agglomerate_affinities(aff, [threshold], 30, device_merge_rounds=rounds, **how)
            assert got.dtype == np.int32
            np.testing.assert_array_equal(got, want, err_msg=f"T {threshold} R {rounds}")
    on_device = inference.agglomerate_affinities(torch.from_numpy(aff).to(dev), [0.7], 30, device_merge_rounds=64,
                                                 return_device_tensor=True, **how)
    assert on_device.device.type == "cuda" and np.array_equal(on_device.cpu().numpy(), want)


def test_float16_affinities(dev):
    """Quantised values: many contacts of count 1 with equal means, the case the strict rule exists for."""
    aff = np.array(watershed_ref.random_affinities("smooth", (17, 17, 65))).astype(np.float16)
    fragments, k = watershed_ref.fragments(aff)
    edges, counts, sums, sizes = region_graph_ref.region_graph(fragments, aff, k)
    means = sums[counts == 1]
    assert len(means) > len(np.unique(means)) > 1                  # count-1 contacts that tie
    for threshold in (0.6, 0.7):
        k, k2 = oracle_first_round(aff, "watershed", threshold)
        assert k2 < k
        want = inference.agglomerate_affinities(aff, [threshold], 30, fragments="watershed")
        for rounds in (1, 64):
            got = inference.agglomerate_affinities(aff, [threshold], 30, fragments="watershed",
                                                   device_merge_rounds=rounds)
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("kind", ["uniform", "smooth"])
def test_with_a_size_floor_the_labels_are_those_of_the_size_floor_alone(dev, kind):
    aff = np.array(watershed_ref.random_affinities(kind, (17, 17, 65)))
    for threshold in (0.6, 0.7):
        k, k2 = oracle_first_round(aff, "watershed", threshold, premerge_size=100)
        assert k2 < k, (k, k2)
        want = inference.agglomerate_affinities(aff, [threshold], 30, fragments="watershed", premerge_size=100)
        for rounds in (1, 64):
            got = inference.agglomerate_affinities(aff, [threshold], 30, fragments="watershed", premerge_size=100,
                                                   device_merge_rounds=rounds)
            np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("threshold", [0.6, 0.7])
def test_end_to_end_at_sixteen_thousand_fragments(dev, threshold):
    """(33, 65, 129) watershed fragments: the device's rounds against the oracle's, then the labels."""
    aff, fragments, k, graph = region_graph_ref.fragment_volume("watershed")
    aff, graph = np.array(aff), tuple(np.array(a) for a in graph)      # the shared ones are read-only
    want_graph, want_map, want_history = dominant_ref.rounds(*graph, threshold)
    assert k >= 10000 and want_history[0] < k and len(want_history) >= 2
    got = inference.contract_dominant_edges(*graph, threshold)
    assert_same(got[:5], want_graph + (want_map,))
    assert got[5] == want_history
    how = dict(fragments="watershed", aff_threshold_low=0.3, aff_threshold_high=0.7)
    want = inference.agglomerate_affinities(aff, [threshold], 0, **how)
    got = inference.agglomerate_affinities(aff, [threshold], 0, device_merge_rounds=64, **how)
    np.testing.assert_array_equal(got, want)
    assert 1 < got.max() < want_history[-1]
