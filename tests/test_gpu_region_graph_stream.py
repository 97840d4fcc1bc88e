"""
The slab-by-slab region graph on the GPU (-m gpu): exaspim_region_graph_stream_slab / _finish,
inference.RegionGraphStream, agglomerate_affinities_streaming and predict_agglomerate_streaming
(DESIGN 6f), bit for bit against the whole-volume numpy oracles (tests/region_graph_ref.py,
tests/components_ref.py) after sorting the edge list by (lo, hi).

The cases are those of tests/test_region_graph_stream_cpu.py, whose numpy model
(tests/region_graph_stream_ref.py) follows the device step for step: seam edges, keys that vanish
because both ids belong to one fragment, keys that pool. Every direct call runs with guard words behind
every buffer, the two carried planes and the counts per id included. Section 8b pushes a slab of more than
twice the tiles one capped launch covers, as the first slab and as the second.
"""

import ctypes

import numpy as np
import pytest
import torch

import components_ref
import region_graph_ref
import region_graph_stream_ref
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

ONE = 1 << 24
GUARD = 64
P64, P32 = -7654321, -1234567      # what every buffer holds before a call
RAGGED = [1, 2, 3, 9, 20, 22]
TILE = (8, 8, 32)
CODES = {torch.float32: _native.AFF_F32, torch.float16: _native.AFF_F16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def every_plane(depth):
    return list(range(1, depth))


def bounds_of(cuts, depth):
    return list(zip([0] + list(cuts), list(cuts) + [depth]))


def capacity_for(n_voxels):
    return 1 << max(6 * n_voxels - 1, 0).bit_length()


def assert_same(got, want):
    for g, w, name in zip(got, want, ("edges", "counts", "sums", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


class Finish:
    """The output buffers of one exaspim_region_graph_stream_finish call, guarded."""

    def __init__(self, dev, capacity, table, n_labels, table_len=None):
        lib = _native.lib()
        self.capacity, self.n_labels = int(capacity), int(n_labels)
        self.table = torch.from_numpy(np.array(table, dtype=np.int32)).to(dev)
        self.table_len = self.table.numel() if table_len is None else int(table_len)
        self.need = lib.exaspim_region_graph_stream_finish_workspace_bytes(self.capacity)
        assert self.need >= 24 * self.capacity, _native.last_error()
        c = self.capacity
        self.edges = torch.full((2 * c + GUARD,), P32, dtype=torch.int32, device=dev)
        self.counts = torch.full((c + GUARD,), P64, dtype=torch.int64, device=dev)
        self.sums = torch.full((c + GUARD,), P64, dtype=torch.int64, device=dev)
        self.sizes = torch.full((self.n_labels + 1 + GUARD,), P64, dtype=torch.int64, device=dev)
        self.state = torch.full((2 + GUARD,), P32, dtype=torch.int32, device=dev)
        self.ws = torch.full((self.need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    NAMES = ["st", "table", "table_len", "n_labels", "edges", "counts", "sums", "sizes", "state", "ws", "need",
             "stream"]

    def args(self, st):
        return [st, self.table.data_ptr(), self.table_len, self.n_labels, self.edges.data_ptr(),
                self.counts.data_ptr(), self.sums.data_ptr(), self.sizes.data_ptr(), self.state.data_ptr(),
                self.ws.data_ptr(), self.need, None]

    def guards_intact(self):
        c = self.capacity
        return bool((self.edges[2 * c:] == P32).all() and (self.counts[c:] == P64).all()
                    and (self.sums[c:] == P64).all() and (self.sizes[self.n_labels + 1:] == P64).all()
                    and (self.state[2:] == P32).all() and (self.ws[self.need:] == 0xA5).all())

    def untouched(self):
        return bool(self.guards_intact() and (self.edges == P32).all() and (self.counts == P64).all()
                    and (self.sums == P64).all() and (self.sizes == P64).all() and (self.state == P32).all()
                    and (self.ws == 0xA5).all())

    def result(self):
        """(edges, counts, sums, sizes) sorted by (lo, hi), and the overflow flag."""
        n_edges, overflow = (int(v) for v in self.state[:2].cpu())
        assert 0 <= n_edges <= self.capacity
        edges = self.edges[:2 * n_edges].cpu().numpy().reshape(-1, 2)
        counts = self.counts[:n_edges].cpu().numpy()
        sums = self.sums[:n_edges].cpu().numpy().view(np.uint64)
        order = np.lexsort((edges[:, 1], edges[:, 0]))
        return (edges[order], counts[order], sums[order], self.sizes[:self.n_labels + 1].cpu().numpy()), overflow


class Stream:
    """A caller of the C ABI: the descriptor and its device buffers, GUARD poisoned words behind each."""

    def __init__(self, dev, shape, id_capacity, edge_capacity):
        self.dev, self.shape = dev, tuple(int(v) for v in shape)
        self.id_capacity, self.capacity = int(id_capacity), int(edge_capacity)
        self.plane = self.shape[1] * self.shape[2]
        c, p = self.capacity, self.plane
        self.keys = torch.full((c + GUARD,), P64, dtype=torch.int64, device=dev)
        self.counts = torch.full((c + GUARD,), P64, dtype=torch.int64, device=dev)
        self.sums = torch.full((c + GUARD,), P64, dtype=torch.int64, device=dev)
        self.sizes_by_id = torch.full((self.id_capacity + 1 + GUARD,), P64, dtype=torch.int64, device=dev)
        self.seam_ids = torch.full((p + GUARD,), P32, dtype=torch.int32, device=dev)
        self.seam_q = torch.full((p + GUARD,), P32, dtype=torch.int32, device=dev)
        self.state = torch.full((2 + GUARD,), P32, dtype=torch.int32, device=dev)
        d = self.desc = _native.RegionGraphStreamDesc()
        d.dims[:] = self.shape
        d.id_capacity, d.edge_capacity, d.next_z = self.id_capacity, self.capacity, 0
        d.keys_dev, d.counts_dev, d.sums_dev = self.keys.data_ptr(), self.counts.data_ptr(), self.sums.data_ptr()
        d.sizes_by_id_dev = self.sizes_by_id.data_ptr()
        d.seam_ids_dev, d.seam_q_dev = self.seam_ids.data_ptr(), self.seam_q.data_ptr()
        d.state_dev = self.state.data_ptr()

    def slab(self, labels, aff, z0):
        """labels, aff: contiguous device tensors of one slab."""
        rc = _native.lib().exaspim_region_graph_stream_slab(
            ctypes.byref(self.desc), labels.data_ptr(), aff.data_ptr(), CODES[aff.dtype],
            _native.int3(labels.shape), z0, None)
        torch.cuda.synchronize()
        return rc

    def push_all(self, labels, aff, cuts):
        """labels (D, H, W) and aff (3, D, H, W) as numpy arrays or device tensors, cut into slabs."""
        if isinstance(labels, np.ndarray):
            labels = torch.from_numpy(np.array(labels, dtype=np.int32, order="C")).to(self.dev)
        if isinstance(aff, np.ndarray):
            aff = torch.from_numpy(np.array(aff, order="C")).to(self.dev)
        for z0, z1 in bounds_of(cuts, self.shape[0]):
            assert self.slab(labels[z0:z1].contiguous(), aff[:, z0:z1].contiguous(), z0) == 0, _native.last_error()
            assert self.desc.next_z == z1
        assert self.guards_intact()
        return self

    def finish(self, table, n_labels, table_len=None):
        f = Finish(self.dev, self.capacity, table, n_labels, table_len)
        rc = _native.lib().exaspim_region_graph_stream_finish(*f.args(ctypes.byref(self.desc)))
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        assert f.guards_intact() and self.guards_intact()
        return f.result()

    def guards_intact(self):
        c, p = self.capacity, self.plane
        return bool((self.keys[c:] == P64).all() and (self.counts[c:] == P64).all() and (self.sums[c:] == P64).all()
                    and (self.sizes_by_id[self.id_capacity + 1:] == P64).all() and (self.seam_ids[p:] == P32).all()
                    and (self.seam_q[p:] == P32).all() and (self.state[2:] == P32).all())

    def untouched(self):
        return bool((self.keys == P64).all() and (self.counts == P64).all() and (self.sums == P64).all()
                    and (self.sizes_by_id == P64).all() and (self.seam_ids == P32).all()
                    and (self.seam_q == P32).all() and (self.state == P32).all())


def provisional_ids(dev, aff_t, fragment_threshold, cuts):
    """A real ComponentsStream with no size filter: the slabs' provisional ids, the stream after finish, K."""
    from aind_exaspim_neuron_segmentation_amd import inference

    vshape = tuple(aff_t.shape[-3:])
    cs = inference.ComponentsStream(vshape, fragment_threshold, 0, device=dev)
    parts = [cs.push(aff_t[:, z0:z1]) for z0, z1 in bounds_of(cuts, vshape[0])]
    table, k = cs.finish()
    return torch.cat(parts), cs, table[: cs.ids_used + 1], k


def streamed_graph(dev, aff, fragment_threshold, cuts, edge_capacity=None):
    """(graph, overflow, final labels, K): ComponentsStream's ids through the C ABI of the graph stream."""
    aff_t = torch.from_numpy(np.array(aff, order="C")).to(dev)
    provisional, cs, table, k = provisional_ids(dev, aff_t, fragment_threshold, cuts)
    st = Stream(dev, aff.shape[1:], cs.id_capacity, edge_capacity or capacity_for(provisional.numel()))
    st.push_all(provisional, aff_t, cuts)
    graph, overflow = st.finish(table.cpu().numpy(), k)
    return graph, overflow, cs.apply(provisional.clone()).cpu().numpy(), k


_WHOLE = {}


def whole(shape, fragment_threshold):
    """(aff, fragments, K, graph): random float32 affinities and the whole volume's oracles, computed once."""
    key = (shape, fragment_threshold)
    if key not in _WHOLE:
        aff = np.random.default_rng(5).random((3,) + shape).astype(np.float32)
        fragments, k = components_ref.components(aff, fragment_threshold, 0)
        graph = region_graph_ref.region_graph(fragments, aff, k)
        for a in (aff, fragments) + graph:
            a.setflags(write=False)
        _WHOLE[key] = (aff, fragments, k, graph)
    return _WHOLE[key]


# ---- 1. against the oracle, provisional ids of a real ComponentsStream ---------------------------
@pytest.mark.parametrize("cuts", [[8, 16], RAGGED, "planes"], ids=["aligned", "ragged", "planes"])
@pytest.mark.parametrize("fragment_threshold", [0.6, 0.75])
@pytest.mark.parametrize("shape", [(23, 37, 71), (24, 40, 72)])
def test_random_affinities_against_the_whole_volume_oracle(dev, shape, fragment_threshold, cuts):
    aff, fragments, k, want = whole(shape, fragment_threshold)
    cuts = every_plane(shape[0]) if cuts == "planes" else cuts
    graph, overflow, final, got_k = streamed_graph(dev, aff, fragment_threshold, cuts)
    assert overflow == 0 and got_k == k
    np.testing.assert_array_equal(final, fragments)
    assert_same(graph, want)


# ---- 2. tables that are no fragment tables ---------------------------------------------------------
def mapped_labels(labels, table, id_capacity, n_labels):
    """What finish makes of every voxel: -1 for what is no id, 0 for what the table does not hold or maps
    outside 0 .. n_labels."""
    ok = (labels >= 0) & (labels <= id_capacity)
    inside = ok & (labels < table.size)
    mapped = np.where(inside, table[np.clip(labels, 0, table.size - 1)], 0)
    mapped = np.where((mapped < 0) | (mapped > n_labels), 0, mapped)
    return np.where(ok, mapped, -1).astype(np.int32)


@pytest.mark.parametrize("cuts", ["planes", [8]], ids=["planes", "cut8"])
@pytest.mark.parametrize("shape", [(9, 10, 37), (17, 8, 33)])
def test_labels_and_tables_that_are_no_fragments(dev, shape, cuts):
    id_capacity, n_labels, table_len = 30, 7, 25
    rng = np.random.default_rng(43)
    labels = rng.integers(0, 41, shape).astype(np.int32)            # 31 .. 40 are beyond id_capacity
    labels[0, 0, :4] = [np.iinfo(np.int32).max, np.iinfo(np.int32).min, -1, -5]
    labels[-1, -1, -3:] = [-2, np.iinfo(np.int32).min, 40]
    labels[shape[0] // 2, 3, 5:8] = [-7, 35, -1]
    aff = whole(shape, 0.75)[0]
    cuts = every_plane(shape[0]) if cuts == "planes" else cuts
    st = Stream(dev, shape, id_capacity, 4096).push_all(labels, aff, cuts)
    for seed in (1, 2):     # the second table on the same accumulator: finish leaves it intact
        table = np.random.default_rng(seed).integers(-1, n_labels + 3, 40).astype(np.int32)   # many to one
        table[0] = 0        # id 0 is every table's background: it forms no edge whatever it maps to
        assert (table[:table_len] == 0).sum() > 1 and (table[:table_len] > n_labels).any()
        assert labels.max() > id_capacity > table_len - 1 and labels.min() < 0
        got, overflow = st.finish(table, n_labels, table_len)
        assert overflow == 0
        want = region_graph_ref.region_graph(mapped_labels(labels, table[:table_len], id_capacity, n_labels), aff,
                                             n_labels)
        assert_same(got, want)
        assert len(want[0]) >= 10 and int(want[3].sum()) == int(((labels >= 0) & (labels <= id_capacity)).sum())


# ---- 3. one key on a whole face ----------------------------------------------------------------------
def test_one_key_on_a_whole_face(dev):
    aff = np.random.default_rng(19).random((3, 3, 64, 64)).astype(np.float32)
    labels = np.empty((3, 64, 64), np.int32)
    labels[0], labels[1], labels[2] = 1, 2, 1
    identity = np.arange(3, dtype=np.int32)
    st = Stream(dev, (2, 64, 64), 2, 64).push_all(labels[:2], aff[:, :2], [1])
    (edges, counts, sums, sizes), overflow = st.finish(identity, 2)
    assert overflow == 0 and edges.tolist() == [[1, 2]] and counts.tolist() == [4096]
    assert sizes.tolist() == [0, 4096, 4096]
    assert int(sums[0]) == int(region_graph_ref.quantise(aff[0, 0]).sum())
    # the carried plane itself
    np.testing.assert_array_equal(st.seam_q[:4096].cpu().numpy().view(np.uint32),
                                  region_graph_ref.quantise(aff[0, 0]).astype(np.uint32).ravel())
    assert (st.seam_ids[:4096] == 1).all()
    st = Stream(dev, (3, 64, 64), 2, 64).push_all(labels, aff, [1, 2])
    (edges, counts, sums, sizes), overflow = st.finish(identity, 2)
    assert overflow == 0 and edges.tolist() == [[1, 2]] and counts.tolist() == [8192]
    assert sizes.tolist() == [0, 8192, 4096]
    assert int(sums[0]) == int(region_graph_ref.quantise(aff[0, :2]).sum())


# ---- 4. every voxel its own label: what finds no LDS slot -----------------------------------------
@pytest.mark.parametrize("shape,cuts", [((9, 10, 37), "planes"), ((9, 64, 64), [8])], ids=["planes", "deep"])
def test_every_voxel_its_own_label(dev, shape, cuts):
    """(9, 64, 64) cut at 8: a full tile of the first slab has some 6000 distinct keys and a workgroup of the
    seam pass 4096, both more than the 2048 slots of the LDS table."""
    n = int(np.prod(shape))
    labels = (np.arange(n, dtype=np.int32) + 1).reshape(shape)
    aff = np.random.default_rng(3).random((3,) + shape).astype(np.float32)
    cuts = every_plane(shape[0]) if cuts == "planes" else cuts
    st = Stream(dev, shape, n, capacity_for(n)).push_all(labels, aff, cuts)
    got, overflow = st.finish(np.arange(n + 1, dtype=np.int32), n)
    assert overflow == 0
    want = region_graph_ref.region_graph(labels, aff, n)
    assert_same(got, want)
    d, h, w = shape
    assert len(want[0]) == 3 * n - (h * w + d * w + d * h) and (want[1] == 1).all() and (want[3][1:] == 1).all()


# ---- 5. what is carried ------------------------------------------------------------------------------
QUANTISATION_EDGES = [0.0, 1.0, 1.5, 1e30, np.inf, -0.25, -np.inf, -0.0, np.nan, 0.5 * 2.0 ** -24,
                      1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24, 0.5 + 0.5 * 2.0 ** -23,
                      0.25 + 1.5 * 2.0 ** -24, 1.0 - 2.0 ** -24, float(np.nextafter(np.float32(1), np.float32(2))),
                      1e-45, 0.3]      # test_gpu_region_graph.test_quantisation_edges


@pytest.mark.parametrize("cuts", [[2], "planes"], ids=["cut2", "planes"])
def test_carried_values(dev, cuts):
    shape = (4, 3, 32)
    n = int(np.prod(shape))
    labels = (np.arange(n, dtype=np.int32) + 1).reshape(shape)      # every edge its own key: sums are per edge
    aff = np.random.default_rng(29).random((3,) + shape).astype(np.float32)
    values = np.array([np.nan, -1.0, 1e30, 0.5 - 2.0 ** -25] + QUANTISATION_EDGES, np.float32)
    aff[0, 1].ravel()[:values.size] = values          # plane 1 is carried across the cut at z = 2
    aff[0, 1, 2, -values.size:] = values[::-1]
    aff[0, -1] = np.nan                               # the volume's last plane carries nothing
    aff[0, -1, ::2] = 1e30
    cuts = every_plane(shape[0]) if cuts == "planes" else cuts
    identity = np.arange(n + 1, dtype=np.int32)
    got, overflow = Stream(dev, shape, n, 4096).push_all(labels, aff, cuts).finish(identity, n)
    assert overflow == 0
    want = region_graph_ref.region_graph(labels, aff, n)
    assert_same(got, want)
    # the z edges below plane 1, by hand
    lo = labels[1].ravel()[:values.size]
    rows = {(int(a), int(b)): int(s) for (a, b), s in zip(got[0], got[2])}
    assert [rows[(int(a), int(a) + 96)] for a in lo] == region_graph_ref.quantise(values).tolist()
    assert rows[(int(lo[3]), int(lo[3]) + 96)] == ONE // 2       # 0.5 - 2^-25 rounds to even
    # float16: equal to the widened float32 input
    half = np.random.default_rng(13).random((3,) + shape).astype(np.float16)
    half[0, 1, 1, 4:9] = [np.nan, 1.5, -2.0, 65504.0, 6e-8]
    half[0, -1] = np.nan
    got16, _ = Stream(dev, shape, n, 4096).push_all(labels, half, cuts).finish(identity, n)
    got32, _ = Stream(dev, shape, n, 4096).push_all(labels, half.astype(np.float32), cuts).finish(identity, n)
    assert_same(got16, got32)
    assert_same(got16, region_graph_ref.region_graph(labels, half, n))


# ---- 6. purity ---------------------------------------------------------------------------------------
def test_cuts_runs_and_capacities_give_the_same_output(dev):
    shape = (17, 8, 33)
    aff, fragments, k, want = whole(shape, 0.75)
    for cuts in ([], [8], [1, 2, 9, 16], every_plane(17)):
        for capacity in (1 << 13, 1 << 16):
            for _ in range(2):
                graph, overflow, final, got_k = streamed_graph(dev, aff, 0.75, cuts, capacity)
                assert overflow == 0 and got_k == k
                assert_same(graph, want)
                np.testing.assert_array_equal(final, fragments)


# ---- 7. overflow -------------------------------------------------------------------------------------
def test_overflow_is_flagged_and_named(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    shape, threshold, capacity = (23, 37, 71), 0.6, 4096
    aff, fragments, k, want = whole(shape, threshold)
    # from the numpy model alone: the provisional keys of the two cut lists around the capacity
    keys = {}
    for name, cuts in (("aligned", [8, 16]), ("planes", every_plane(23))):
        keys[name] = region_graph_stream_ref.fragments_streamed(aff, threshold, cuts)[2].keys.size
    assert keys == {"aligned": 2535, "planes": 50825} and keys["aligned"] < capacity < keys["planes"]
    assert len(want[0]) == 1066 < capacity
    graph, overflow, final, _ = streamed_graph(dev, aff, threshold, [8, 16], capacity)     # asserts the guards
    assert overflow == 0
    assert_same(graph, want)
    _, overflow, _, _ = streamed_graph(dev, aff, threshold, every_plane(23), capacity)     # asserts the guards
    assert overflow == 1
    aff_t = torch.from_numpy(aff.copy()).to(dev)
    for cuts in ([8, 16], every_plane(23)):
        provisional, cs, table, got_k = provisional_ids(dev, aff_t, threshold, cuts)
        rgs = inference.RegionGraphStream(shape, device=dev, edge_capacity=capacity)
        for z0, z1 in bounds_of(cuts, 23):
            rgs.push(provisional[z0:z1], aff_t[:, z0:z1], z0)
        if len(cuts) == 2:
            assert_same(rgs.finish(table, got_k), want)
        else:
            with pytest.raises(RuntimeError, match="edge_capacity=4096.*[Ss]hallow slabs"):
                rgs.finish(table, got_k)


# ---- 8. 64-bit sizes ---------------------------------------------------------------------------------
def test_sizes_are_summed_in_64_bits(dev):
    shape = (2, 2, 4)
    labels = np.zeros(shape, np.int32)
    labels[0, 0, :2], labels[1, 1, 2:] = 1, 2
    aff = np.full((3,) + shape, 0.5, np.float32)
    st = Stream(dev, shape, 5, 64).push_all(labels, aff, [1])
    assert st.sizes_by_id[:6].tolist() == [12, 2, 2, 0, 0, 0]
    st.sizes_by_id[1:3] = 1_500_000_000
    (edges, _, _, sizes), overflow = st.finish(np.array([0, 3, 3, 1, 1, 1], np.int32), 3)
    assert overflow == 0 and len(edges) == 0
    assert sizes.tolist() == [12, 0, 0, 3_000_000_000]


# ---- 8b. a slab of more tiles than one capped launch covers -------------------------------------------
@pytest.mark.parametrize("cuts", [[560003], [3]], ids=["first", "second"])
def test_grid_stride_over_the_tiles_of_a_slab(dev, cuts):
    """
    The volume of test_gpu_region_graph.test_grid_stride_over_tiles (147 456 tiles) in two slabs, against the
    whole volume's oracle. Cut at 560003 the slab that resets the table has 140 002 tiles and the seam lies
    at a plane that is no multiple of 8; cut at 3 the striding slab is the second one, which adds to a table
    it did not reset and to the voxel counts of the first.
    """
    labels, aff, k, want, _ = region_graph_ref.stride_volume()
    shape = labels.shape
    z0, z1 = max(bounds_of(cuts, shape[0]), key=lambda b: b[1] - b[0])
    assert -(-(z1 - z0) // TILE[0]) * -(-shape[1] // TILE[1]) * -(-shape[2] // TILE[2]) >= 2 * 65536
    assert (z0 == 0) == (cuts == [560003]) and cuts[0] % TILE[0] != 0
    capacity = 1 << (4 * len(want[0]) - 1).bit_length()
    st = Stream(dev, shape, k, capacity).push_all(labels, aff, cuts)
    got, overflow = st.finish(np.arange(k + 1, dtype=np.int32), k)      # asserts the guards
    assert overflow == 0
    assert_same(got, want)


# ---- 9. refusals, before anything is launched ----------------------------------------------------------
def test_refusals(dev):
    lib = _native.lib()
    shape = (9, 10, 37)
    aff, fragments, k, want = whole(shape, 0.75)
    st = Stream(dev, shape, k, 4096)
    labels_t = torch.from_numpy(fragments.copy()).to(dev)
    aff_t = torch.from_numpy(aff.copy()).to(dev)
    half_t = aff_t.half()
    aff4 = aff_t[:, :4].contiguous()
    big = Finish(dev, 4096, np.arange(k + 1, dtype=np.int32), k)
    fields = ["keys_dev", "counts_dev", "sums_dev", "sizes_by_id_dev", "seam_ids_dev", "seam_q_dev", "state_dev"]

    def desc_with(**changes):
        d = _native.RegionGraphStreamDesc()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(st.desc), ctypes.sizeof(d))
        for name, value in changes.items():
            if name == "dims":
                d.dims[:] = value
            else:
                setattr(d, name, value)
        return d

    def slab_refused(what, desc=None, **changes):
        d = st.desc if desc is None else desc
        before = bytes(d)
        args = dict(st=ctypes.byref(d), labels=labels_t[:4].data_ptr(), aff=aff4.data_ptr(),
                    dtype=_native.AFF_F32, dims=_native.int3((4,) + shape[1:]), z0=d.next_z, stream=None)
        args.update(changes)
        rc = lib.exaspim_region_graph_stream_slab(*args.values())
        torch.cuda.synchronize()
        assert rc == -1, (what, changes, _native.last_error())
        assert what in _native.last_error(), (what, changes, _native.last_error())
        assert bytes(d) == before and st.untouched() and big.untouched(), (what, changes)

    def finish_refused(code, what, desc=None, **changes):
        d = st.desc if desc is None else desc
        before = bytes(d)
        args = big.args(ctypes.byref(d))
        for name, value in changes.items():
            args[Finish.NAMES.index(name)] = value
        rc = lib.exaspim_region_graph_stream_finish(*args)
        torch.cuda.synchronize()
        assert rc == code, (what, changes, _native.last_error())
        assert what in _native.last_error(), (what, changes, _native.last_error())
        assert bytes(d) == before and st.untouched() and big.untouched(), (what, changes)

    def both_refused(what, desc):
        slab_refused(what, desc)
        finish_refused(-1, what, desc)

    # the slab call's own arguments
    for name in ("st", "labels", "aff"):      # the binding's int32[3] type cannot hold a NULL slab_dims
        slab_refused("NULL", **{name: None})
    slab_refused("aff_dtype", dtype=2)
    slab_refused("aff_dtype", dtype=-1)
    slab_refused("misaligned", labels=labels_t.data_ptr() + 2)
    slab_refused("misaligned", aff=aff_t.data_ptr() + 2)
    slab_refused("misaligned", aff=half_t.data_ptr() + 1, dtype=_native.AFF_F16)
    slab_refused("slab_dims", dims=_native.int3((0, 10, 37)))
    slab_refused("slab_dims", dims=_native.int3((4, -10, 37)))
    slab_refused("(y, x)", dims=_native.int3((4, 37, 10)))
    slab_refused("(y, x)", dims=_native.int3((4, 10, 36)))
    slab_refused("out of order", z0=1)
    slab_refused("out of order", z0=-1)
    slab_refused("beyond the volume", dims=_native.int3((10, 10, 37)))
    slab_refused("out of order", desc_with(next_z=5), z0=0)
    slab_refused("beyond the volume", desc_with(next_z=6))
    # a slab of 2^31 voxels in a volume that may have them
    slab_refused("slab_dims", desc_with(dims=[4096, 1024, 1024]), dims=_native.int3((2048, 1024, 1024)))
    # the descriptor, for both calls
    for name in fields:
        both_refused("NULL", desc_with(**{name: None}))
        both_refused("misaligned", desc_with(**{name: getattr(st.desc, name) + 2}))
    for name in ("keys_dev", "counts_dev", "sums_dev", "sizes_by_id_dev"):
        both_refused("misaligned", desc_with(**{name: getattr(st.desc, name) + 4}))
    for capacity in (0, -4096, 4095, 3 << 10, (1 << 30) + 1, 1 << 31):
        both_refused("edge_capacity", desc_with(edge_capacity=capacity))
        assert lib.exaspim_region_graph_stream_finish_workspace_bytes(capacity) == 0
        assert "edge_capacity" in _native.last_error()
    for capacity in (0, -1, 2**31 - 1):
        both_refused("id_capacity", desc_with(id_capacity=capacity))
    both_refused("dims", desc_with(dims=[9, 0, 37]))
    both_refused("dims", desc_with(dims=[-9, 10, 37]))
    both_refused("plane", desc_with(dims=[9, 65536, 32768]))
    both_refused("next_z", desc_with(next_z=-1))
    both_refused("next_z", desc_with(next_z=10))
    # finish
    finish_refused(-1, "before the last plane")                       # nothing was pushed
    finish_refused(-1, "before the last plane", desc_with(next_z=8))
    done = desc_with(next_z=9)
    finish_refused(-1, "NULL", None, st=None)
    for name in ("table", "edges", "counts", "sums", "sizes", "state", "ws"):
        finish_refused(-1, "NULL", done, **{name: None})
    finish_refused(-1, "table_len", done, table_len=0)
    finish_refused(-1, "table_len", done, table_len=-3)
    finish_refused(-1, "n_labels", done, n_labels=-1)
    finish_refused(-1, "misaligned", done, table=big.table.data_ptr() + 2)
    finish_refused(-1, "misaligned", done, edges=big.edges.data_ptr() + 2)
    finish_refused(-1, "misaligned", done, counts=big.counts.data_ptr() + 4)
    finish_refused(-1, "misaligned", done, sums=big.sums.data_ptr() + 4)
    finish_refused(-1, "misaligned", done, sizes=big.sizes.data_ptr() + 4)
    finish_refused(-1, "misaligned", done, state=big.state.data_ptr() + 2)
    finish_refused(-1, "misaligned", done, ws=big.ws.data_ptr() + 8)
    finish_refused(-3, "workspace", done, need=big.need - 1)
    # and the same buffers do serve a sound run afterwards
    assert st.desc.next_z == 0
    st.push_all(labels_t, aff_t, [4])
    got, overflow = st.finish(np.arange(k + 1, dtype=np.int32), k)
    assert overflow == 0
    assert_same(got, want)
    # a second push of the last slab
    aff5 = aff_t[:, 4:].contiguous()
    rc = lib.exaspim_region_graph_stream_slab(ctypes.byref(st.desc), labels_t[4:].data_ptr(), aff5.data_ptr(), 0,
                                              _native.int3((5, 10, 37)), 4, None)
    assert rc == -1 and "out of order" in _native.last_error() and st.desc.next_z == 9


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    shape = (9, 10, 37)
    aff, fragments, k, want = whole(shape, 0.75)
    labels_t = torch.from_numpy(fragments.copy()).to(dev)
    aff_t = torch.from_numpy(aff.copy()).to(dev)
    table = torch.arange(k + 1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="edge_capacity"):
        inference.RegionGraphStream(shape, device=dev, edge_capacity=1000)
    with pytest.raises(ValueError, match="id_capacity"):
        inference.RegionGraphStream(shape, device=dev, id_capacity=0)
    with pytest.raises(ValueError, match="shape"):
        inference.RegionGraphStream((9, 10), device=dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.RegionGraphStream(shape, device="cpu")
    rgs = inference.RegionGraphStream(shape, device=dev)
    assert rgs.id_capacity == 9 * 10 * 37 and rgs.edge_capacity == inference._default_edge_capacity(9 * 10 * 37)
    with pytest.raises(TypeError):
        rgs.push(fragments[:4], aff_t[:, :4])
    with pytest.raises(TypeError, match="int32"):
        rgs.push(labels_t[:4].long(), aff_t[:, :4])
    with pytest.raises(TypeError, match="float32 or float16"):
        rgs.push(labels_t[:4], aff_t[:, :4].double())
    with pytest.raises(RuntimeError, match="cpu"):
        rgs.push(labels_t[:4].cpu(), aff_t[:, :4])
    with pytest.raises(ValueError, match="no affinities to score"):
        rgs.push(labels_t[:4], aff_t[0, :4])
    with pytest.raises(ValueError, match="labels must be"):
        rgs.push(labels_t[:3], aff_t[:, :4])
    with pytest.raises(ValueError, match="out of order"):
        rgs.push(labels_t[:4], aff_t[:, :4], z0=2)
    with pytest.raises(ValueError, match=r"\(y, x\)"):
        rgs.push(labels_t[:4, :, :36], aff_t[:, :4, :, :36])
    with pytest.raises(RuntimeError, match="0 of 9 planes"):
        rgs.finish(table, k)
    assert rgs.next_z == 0
    rgs.push(labels_t[:4], aff_t[:, :4], z0=0)
    with pytest.raises(ValueError, match="beyond the volume"):
        rgs.push(labels_t[3:], aff_t[:, 3:])
    assert rgs.next_z == 4
    rgs.push(labels_t[4:], aff_t[:, 4:])
    assert rgs.next_z == 9
    with pytest.raises(TypeError, match="int32"):
        rgs.finish(table.long(), k)
    with pytest.raises(ValueError, match="n_labels"):
        rgs.finish(table, -1)
    assert_same(rgs.finish(table, k), want)
    assert_same(rgs.finish(table.cpu().numpy(), k), want)            # again, and with a numpy table
    with pytest.raises(ValueError, match="no affinities to score"):
        inference.agglomerate_affinities_streaming(aff[0], slab_depth=4)
    with pytest.raises(ValueError, match="non-decreasing"):
        inference.agglomerate_affinities_streaming(aff, [0.9, 0.8], slab_depth=4)
    with pytest.raises(ValueError, match="slab_depth"):
        inference.agglomerate_affinities_streaming(aff, slab_depth=0)
    with pytest.raises(TypeError, match="float32 or float16"):
        inference.agglomerate_affinities_streaming(aff.astype(np.float64), slab_depth=4)


# ---- 10. end to end ------------------------------------------------------------------------------------
def collect(blocks):
    return lambda z0, z1, block: blocks.append((z0, z1, block.dtype, block.shape, block.copy()))


@pytest.mark.parametrize("shape", [(9, 10, 37), (17, 8, 33)])
def test_agglomerate_affinities_streaming_on_random_affinities(dev, shape):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, _, k, _ = whole(shape, 0.75)
    partly = False
    for thresholds, min_size in (([0.55], 0), ([0.5, 0.6], 0), ([0.6], 10), ([0.9], 0)):
        want = region_graph_ref.agglomerate_affinities(aff, thresholds, min_size, 0.75)
        np.testing.assert_array_equal(inference.agglomerate_affinities(aff, thresholds, min_size,
                                                                       fragment_threshold=0.75), want)
        partly = partly or 1 < int(want.max()) < k
        for slab_depth in (1, 4, 7):
            for resident in (True, False):
                got = inference.agglomerate_affinities_streaming(aff, thresholds, min_size, fragment_threshold=0.75,
                                                                 slab_depth=slab_depth, keep_labels_resident=resident)
                assert isinstance(got, np.ndarray) and got.dtype == np.int32
                np.testing.assert_array_equal(got, want)
            blocks = []
            table, s = inference.agglomerate_affinities_streaming(aff, thresholds, min_size, fragment_threshold=0.75,
                                                                  slab_depth=slab_depth, write_block=collect(blocks))
            assert [(b[0], b[1]) for b in blocks] == [(z, min(z + slab_depth, shape[0]))
                                                      for z in range(0, shape[0], slab_depth)]
            assert all(b[2] == np.int32 and b[3] == (b[1] - b[0],) + shape[1:] for b in blocks)
            provisional = np.concatenate([b[4] for b in blocks])
            assert table.dtype == np.int32 and table[0] == 0 and provisional.max() == table.size - 1
            np.testing.assert_array_equal(table[provisional], want)
            assert s == int(want.max())
    assert partly
    half = aff.astype(np.float16)
    want = region_graph_ref.agglomerate_affinities(half, [0.6], 5, 0.75)
    np.testing.assert_array_equal(
        inference.agglomerate_affinities_streaming(half, [0.6], 5, fragment_threshold=0.75, slab_depth=4), want)


def test_agglomerate_affinities_streaming_with_the_defaults(dev, golden):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = golden("g10_components.npz")["aff"].astype(np.float32)
    fragments, k = components_ref.components(aff, 0.5, 0)
    assert k <= 64                     # keeps the naive oracle quick
    want = region_graph_ref.agglomerate_affinities(aff)
    np.testing.assert_array_equal(inference.agglomerate_affinities(aff), want)
    for resident in (True, False):
        got = inference.agglomerate_affinities_streaming(aff, slab_depth=5, keep_labels_resident=resident)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    blocks = []
    table, s = inference.agglomerate_affinities_streaming(aff, slab_depth=5, write_block=collect(blocks))
    np.testing.assert_array_equal(table[np.concatenate([b[4] for b in blocks])], want)
    assert s == int(want.max())


SEAM = 28
GEOMETRY = dict(batch_size=3, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4, verbose=False)


def seam_cases(aff):
    """
    Fragment and agglomeration thresholds from predict_streaming's own output, with their oracles.

    This model's outputs lie in three narrow bands, one per channel (z about 0.446, x about 0.486, y about
    0.553, the z channel with a thin tail up to 0.49), so below the x band every plane of the predicted
    region is one fragment and planes are joined by the few z edges of that tail: the fragments of planes
    27 and 28 are either one fragment, which then has voxels on both sides of the seam, or two, whose
    contact then has a whole plane of voxel edges across it -- never both at one threshold. So there are two
    cases, each the first quantile of the z channel's upper tail with its property and with fragments few
    enough for the naive oracle:
        joined   a fragment has voxels on both sides of z = 28 (the seam unites provisional ids);
        apart    a contact has voxel edges across z = 28 (the seam adds to the graph).
    Both are merged where a contact's mean is above the median contact's, as
    test_gpu_region_graph.test_predict_device_tensor_feeds_agglomeration does.
    """
    tail = aff[0, :-1]
    cases, tried = {}, []
    for q in (0.999, 0.9993, 0.9995, 0.9997, 0.9998, 0.9999, 0.99995, 0.99, 0.9, 0.6):
        fragment_threshold = float(np.quantile(tail, q))
        fragments, k = components_ref.components(aff, fragment_threshold, 0)
        both = np.intersect1d(fragments[:SEAM], fragments[SEAM:])
        above, below = fragments[SEAM - 1], fragments[SEAM]
        across = int(((above > 0) & (below > 0) & (above != below)).sum())
        tried.append((q, fragment_threshold, k, int((both > 0).sum()), across))
        for name, holds in (("joined", (both > 0).any()), ("apart", across >= 1)):
            if name in cases or not holds or not 2 <= k <= 2000:
                continue
            edges, counts, sums, sizes = region_graph_ref.region_graph(fragments, aff, k)
            if not 1 <= len(edges) <= 5000:
                continue
            means = np.sort(sums.astype(np.float64) / counts / ONE)
            threshold = 1.0 - float(means[len(means) // 2])
            want = {}
            for min_size in (0, 20):
                table, s = region_graph_ref.agglomerate(edges, counts, sums, sizes, threshold, min_size)
                want[min_size] = (table[fragments], s)
            if 1 <= want[0][1] < k:
                cases[name] = dict(fragment_threshold=fragment_threshold, threshold=threshold, k=k, want=want,
                                   crossing=int((both > 0).sum()), across=across)
        if len(cases) == 2:
            break
    print("quantile of the z channel, fragment threshold, K, fragments on both sides of z = 28, voxel edges of "
          "contacts across it:", tried)
    return cases


@pytest.fixture(scope="module")
def e2e(dev):
    """The tiny model and geometry of test_gpu_components_stream.e2e (two finished slabs, one seam at
    z = 28), predict_streaming's own affinities and the two cases of seam_cases."""
    from aind_exaspim_neuron_segmentation_amd import inference
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, 0.125, seed=1)
    model = UNet3D(output_channels=3, width_multiplier=0.125)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to(dev).eval()
    vol = synthetic.synth_volume((40, 48, 56), seed=21)
    aff = inference.predict_streaming(vol, model, **GEOMETRY)
    assert aff.dtype == np.float32 and aff.shape == (3, 40, 48, 56)
    cases = seam_cases(aff)
    assert sorted(cases) == ["apart", "joined"], cases.keys()
    assert cases["joined"]["crossing"] >= 1 and cases["apart"]["across"] >= 1
    for case in cases.values():
        assert 1 <= case["want"][0][1] < case["k"]       # merging ends strictly between one segment and none merged
    return dict(model=model, vol=vol, aff=aff, cases=cases)


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("name", ["joined", "apart"])
def test_predict_agglomerate_streaming_equals_the_oracle(dev, e2e, name, resident):
    from aind_exaspim_neuron_segmentation_amd import inference

    case = e2e["cases"][name]
    for min_size, (want, s) in case["want"].items():
        timings = {}
        got = inference.predict_agglomerate_streaming(e2e["vol"], e2e["model"], [case["threshold"]], min_size,
                                                      fragment_threshold=case["fragment_threshold"],
                                                      keep_labels_resident=resident, timings=timings, **GEOMETRY)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
        assert int(got.max()) == s
        assert timings["agglomerate_finish"] > 0 and "layers" in timings


@pytest.mark.parametrize("name", ["joined", "apart"])
def test_predict_agglomerate_streaming_write_block(dev, e2e, name):
    from aind_exaspim_neuron_segmentation_amd import inference

    case = e2e["cases"][name]
    blocks = []
    want, s = case["want"][20]
    kw = dict(fragment_threshold=case["fragment_threshold"])
    table, got_s = inference.predict_agglomerate_streaming(e2e["vol"], e2e["model"], [case["threshold"]], 20,
                                                           write_block=collect(blocks), **kw, **GEOMETRY)
    assert [(b[0], b[1]) for b in blocks] == [(0, SEAM), (SEAM, 40)]       # two slabs, one seam
    assert all(b[2] == np.int32 and b[3] == (b[1] - b[0], 48, 56) for b in blocks)   # int32 and nothing else left
    provisional = np.concatenate([b[4] for b in blocks])
    assert table.dtype == np.int32 and table[0] == 0 and provisional.max() < table.size
    np.testing.assert_array_equal(table[provisional], want)
    assert got_s == s
    # the same through the host-array form and the whole-volume form, on predict_streaming's own output
    got = inference.agglomerate_affinities_streaming(e2e["aff"], [case["threshold"]], 20, slab_depth=7, **kw)
    np.testing.assert_array_equal(got, want)
    got = inference.agglomerate_affinities(e2e["aff"], [case["threshold"]], 20, **kw)
    np.testing.assert_array_equal(got, want)


def test_a_foreground_map_is_refused(dev, e2e):
    from aind_exaspim_neuron_segmentation_amd import inference

    with pytest.raises(ValueError, match="no affinities to score"):
        inference.predict_agglomerate_streaming(e2e["vol"], e2e["model"], affinity_mode=False, **GEOMETRY)
