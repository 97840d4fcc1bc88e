"""
exaspim_region_graph, exaspim_apply_label_table and inference.agglomerate_affinities on the GPU
(-m gpu), bit for bit against the numpy oracles of tests/region_graph_ref.py after sorting the edge
list by (lo, hi).

The kernel reduces 8 x 8 x 32 tiles (with a +1 halo) in an LDS table of 2048 slots and flushes one
update per distinct key and tile into the global table; what finds no LDS slot goes to the global
table directly. The shapes sit around the tile; "every voxel its own label" has about three distinct
pairs per voxel, 6000 per tile, so the LDS table overflows; two slabs put all contention on one slot.
Every direct call runs with guard words behind every buffer. The last section runs agglomerate_affinities
and its streamed form at 16 115 watershed and 27 082 component fragments against the heap oracle
(region_graph_ref.agglomerate_fast, itself held to the naive one in tests/test_agglomerate_scale_cpu.py);
section 14 a long thin volume of 147 456 tiles, more than twice what one capped launch covers, in both
affinity types.
"""

import numpy as np
import pytest
import torch

import components_ref
import region_graph_ref
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

ONE = 1 << 24
GUARD = 64
TILE = (8, 8, 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def capacity_for(n_voxels):
    return 1 << max(6 * n_voxels - 1, 0).bit_length()


class Call:
    """One exaspim_region_graph call: every buffer with GUARD poisoned words behind it."""

    def __init__(self, dev, labels, aff, n_labels, capacity):
        lib = _native.lib()
        self.shape = tuple(labels.shape)
        self.n_labels, self.capacity = int(n_labels), int(capacity)
        self.labels = torch.from_numpy(np.array(labels, dtype=np.int32, order="C")).to(dev)
        self.aff = torch.from_numpy(np.array(aff, order="C")).to(dev)
        self.code = {torch.float32: _native.AFF_F32, torch.float16: _native.AFF_F16}[self.aff.dtype]
        self.dims = _native.int3(self.shape)
        self.need = lib.exaspim_region_graph_workspace_bytes(self.dims, self.n_labels, self.capacity)
        assert self.need >= 24 * self.capacity, _native.last_error()
        c = self.capacity
        self.edges = torch.full((2 * c + GUARD,), -1234567, dtype=torch.int32, device=dev)
        self.counts = torch.full((c + GUARD,), -7654321, dtype=torch.int64, device=dev)
        self.sums = torch.full((c + GUARD,), -1111111, dtype=torch.int64, device=dev)
        self.sizes = torch.full((self.n_labels + 1 + GUARD,), -2222222, dtype=torch.int64, device=dev)
        self.state = torch.full((2 + GUARD,), -3333333, dtype=torch.int32, device=dev)
        self.ws = torch.full((self.need + GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    def args(self):
        return [self.labels.data_ptr(), self.aff.data_ptr(), self.code, self.dims, self.n_labels, self.capacity,
                self.edges.data_ptr(), self.counts.data_ptr(), self.sums.data_ptr(), self.sizes.data_ptr(),
                self.state.data_ptr(), self.ws.data_ptr(), self.need, None]

    def run(self, args=None):
        rc = _native.lib().exaspim_region_graph(*(self.args() if args is None else args))
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        c = self.capacity
        return bool((self.edges[2 * c:] == -1234567).all() and (self.counts[c:] == -7654321).all()
                    and (self.sums[c:] == -1111111).all() and (self.sizes[self.n_labels + 1:] == -2222222).all()
                    and (self.state[2:] == -3333333).all() and (self.ws[self.need:] == 0xA5).all())

    def untouched(self):
        c = self.capacity
        return bool(self.guards_intact() and (self.edges[:2 * c] == -1234567).all()
                    and (self.counts[:c] == -7654321).all() and (self.sums[:c] == -1111111).all()
                    and (self.sizes[:self.n_labels + 1] == -2222222).all() and (self.state[:2] == -3333333).all()
                    and (self.ws[:self.need] == 0xA5).all())

    def result(self):
        """(edges, counts, sums, sizes) sorted by (lo, hi), and the overflow flag."""
        n_edges, overflow = (int(v) for v in self.state[:2].cpu())
        assert 0 <= n_edges <= self.capacity
        edges = self.edges[:2 * n_edges].cpu().numpy().reshape(-1, 2)
        counts = self.counts[:n_edges].cpu().numpy()
        sums = self.sums[:n_edges].cpu().numpy().view(np.uint64)
        order = np.lexsort((edges[:, 1], edges[:, 0]))
        return (edges[order], counts[order], sums[order], self.sizes[:self.n_labels + 1].cpu().numpy()), overflow


def device_graph(dev, labels, aff, n_labels, capacity=None):
    call = Call(dev, labels, aff, n_labels, capacity or capacity_for(labels.size))
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact()
    got, overflow = call.result()
    assert overflow == 0
    return got


def assert_same(got, want):
    for g, w, name in zip(got, want, ("edges", "counts", "sums", "sizes")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=name)


def check(dev, labels, aff, n_labels, capacity=None):
    want = region_graph_ref.region_graph(labels, aff, n_labels)
    assert_same(device_graph(dev, labels, aff, n_labels, capacity), want)
    return want


_RANDOM = {}


def random_case(shape, fragment_threshold=0.75):
    """(aff, fragments, K): random float32 affinities and the oracle's fragments, computed once."""
    key = (shape, fragment_threshold)
    if key not in _RANDOM:
        aff = np.random.default_rng(5).random((3,) + shape).astype(np.float32)
        fragments, k = components_ref.components(aff, fragment_threshold, 0)
        aff.setflags(write=False)
        fragments.setflags(write=False)
        _RANDOM[key] = (aff, fragments, k)
    return _RANDOM[key]


# ---- 1. random affinities, the oracle's fragments, shapes around the tile --------------------------
@pytest.mark.parametrize("shape", [(9, 10, 37), (17, 8, 33), (8, 8, 32), (1, 1, 2), (1, 5, 1), (2, 64, 64)])
def test_random_affinities_with_the_oracles_fragments(dev, shape):
    for fragment_threshold in (0.75, 0.5):
        aff, fragments, k = random_case(shape, fragment_threshold)
        edges, counts, sums, sizes = check(dev, fragments, aff, k)
        np.testing.assert_array_equal(sizes, np.bincount(fragments.ravel(), minlength=k + 1))
        if min(shape) > 1:
            assert k >= 2 and len(edges) >= 1 and int(counts.max()) >= 2
    # labels that are no fragments at all: independent of the affinities, every id next to every other
    rng = np.random.default_rng(31)
    labels = rng.integers(0, 6, shape).astype(np.int32)
    edges, counts, _, sizes = check(dev, labels, random_case(shape)[0], 5)
    np.testing.assert_array_equal(sizes, np.bincount(labels.ravel(), minlength=6))
    if np.prod(shape) >= 2048:
        assert len(edges) == 10


# ---- 2. float16 ----------------------------------------------------------------------------------
def test_float16_equals_the_widened_float32(dev):
    shape = (9, 10, 37)
    _, fragments, k = random_case(shape)
    half = np.random.default_rng(13).random((3,) + shape).astype(np.float16)
    half[:, 2, 3, 4:9] = [np.nan, 1.5, -2.0, 65504.0, 6e-8]
    got16 = device_graph(dev, fragments, half, k)
    got32 = device_graph(dev, fragments, half.astype(np.float32), k)
    assert_same(got16, got32)
    assert_same(got16, region_graph_ref.region_graph(fragments, half, k))


# ---- 3. every voxel its own label: the LDS table overflows ----------------------------------------
def test_every_voxel_its_own_label(dev):
    shape = (8, 16, 64)
    n = int(np.prod(shape))
    labels = (np.arange(n, dtype=np.int32) + 1).reshape(shape)
    aff = np.random.default_rng(3).random((3,) + shape).astype(np.float32)
    edges, counts, sums, sizes = check(dev, labels, aff, n)
    n_pairs = 3 * n - (16 * 64 + 8 * 64 + 8 * 16)
    assert len(edges) == n_pairs > 4 * 2048 and (counts == 1).all() and (sizes[1:] == 1).all() and sizes[0] == 0
    # a table with fewer slots than pairs: the flag goes up, the call returns, nothing is written past a buffer
    call = Call(dev, labels, aff, n, 1024)
    assert call.run() == 0, _native.last_error()
    assert call.guards_intact()
    _, overflow = call.result()
    assert overflow == 1


def test_overflow_raises_an_error_that_names_edge_capacity(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    shape = (8, 16, 64)
    labels = (np.arange(int(np.prod(shape)), dtype=np.int32) + 1).reshape(shape)
    aff = np.full((3,) + shape, 0.5, np.float32)
    with pytest.raises(RuntimeError, match="edge_capacity=1024"):
        inference.region_graph(labels, aff, edge_capacity=1024)
    # the table exactly as large as the number of pairs still holds them
    n_pairs = 3 * labels.size - (16 * 64 + 8 * 64 + 8 * 16)
    edges, counts, sums, sizes = inference.region_graph(labels, aff, edge_capacity=32768)
    assert len(edges) == n_pairs <= 32768 and (sums == ONE // 2).all()


# ---- 4. two slabs that meet in one face: all contention on one slot ------------------------------
def test_two_slabs_meet_in_one_face(dev):
    shape = (2, 64, 64)
    labels = np.empty(shape, np.int32)
    labels[0], labels[1] = 1, 2
    aff = np.random.default_rng(19).random((3,) + shape).astype(np.float32)
    edges, counts, sums, sizes = check(dev, labels, aff, 2)
    assert edges.tolist() == [[1, 2]] and counts.tolist() == [4096] and sizes.tolist() == [0, 4096, 4096]
    assert int(sums[0]) == int(region_graph_ref.quantise(aff[0, 0]).sum())
    # the same contact along x, where a tile sees 64 of its edges, and across many tiles along z
    shape = (40, 9, 34)
    labels = np.ones(shape, np.int32)
    labels[:, :, 17:] = 2
    aff = np.random.default_rng(23).random((3,) + shape).astype(np.float32)
    edges, counts, _, _ = check(dev, labels, aff, 2)
    assert edges.tolist() == [[1, 2]] and counts.tolist() == [40 * 9]


# ---- 5. what is no label -------------------------------------------------------------------------
def test_labels_outside_the_range_are_ignored(dev):
    shape = (9, 10, 37)
    rng = np.random.default_rng(37)
    labels = rng.integers(-3, 10, shape).astype(np.int32)
    labels[0, 0, :4] = [np.iinfo(np.int32).max, np.iinfo(np.int32).min, 7, -1]
    aff = random_case(shape)[0]
    edges, counts, sums, sizes = check(dev, labels, aff, 6)
    assert edges.max() == 6 and edges.min() == 1 and len(edges) == 15
    assert int(sizes.sum()) == int(((labels >= 0) & (labels <= 6)).sum()) < labels.size
    # the same voxels as background from the start: the same graph
    clean = np.where((labels < 0) | (labels > 6), 0, labels).astype(np.int32)
    got = device_graph(dev, clean, aff, 6)
    assert_same(got[:3], (edges, counts, sums))
    # no labels at all
    edges, _, _, sizes = check(dev, np.zeros(shape, np.int32), aff, 0)
    assert len(edges) == 0 and sizes.tolist() == [labels.size]


# ---- 6. entries that leave the volume --------------------------------------------------------------
def test_high_face_entries_are_ignored(dev):
    shape = (9, 17, 35)
    aff, fragments, k = random_case(shape)
    base = device_graph(dev, fragments, aff, k)
    hot = aff.copy()
    hot[0, -1], hot[1, :, -1] = np.nan, 1e30
    hot[2, :, :, -1] = np.nan
    hot[2, ::2, :, -1] = 1e30
    assert_same(device_graph(dev, fragments, hot, k), base)
    assert_same(base, region_graph_ref.region_graph(fragments, hot, k))


# ---- 7. q's edges ----------------------------------------------------------------------------------
def test_quantisation_edges(dev):
    half = 2.0 ** -24
    values = np.array([0.0, 1.0, 1.5, 1e30, np.inf, -0.25, -np.inf, -0.0, np.nan, 0.5 * half, 1.5 * half,
                       2.5 * half, 3.5 * half, 0.5 + 0.5 * 2.0 ** -23, 0.25 + 1.5 * half, 1.0 - 2.0 ** -24,
                       np.nextafter(np.float32(1), np.float32(2)), 1e-45, 0.3], np.float32)
    want = [0, ONE, ONE, ONE, ONE, 0, 0, 0, 0, 0, 2, 2, 4, ONE // 2 + 1, ONE // 4 + 2, ONE - 1, ONE, 0,
            int(np.rint(np.float32(0.3) * np.float32(ONE)))]
    assert region_graph_ref.quantise(values).tolist() == want
    # a row of voxels, each its own label: edge (i + 1, i + 2) carries values[i]
    n = values.size + 1
    labels = (np.arange(n, dtype=np.int32) + 1).reshape(1, 1, n)
    aff = np.zeros((3, 1, 1, n), np.float32)
    aff[2, 0, 0, :-1] = values
    aff[2, 0, 0, -1] = 0.7      # leaves the volume
    edges, counts, sums, _ = check(dev, labels, aff, n)
    assert edges[:, 0].tolist() == list(range(1, n)) and (counts == 1).all()
    assert sums.tolist() == want


# ---- 8. purity -----------------------------------------------------------------------------------
def test_two_runs_and_two_capacities_give_the_same_output(dev):
    shape = (17, 8, 33)
    aff, fragments, k = random_case(shape)
    base = device_graph(dev, fragments, aff, k)
    assert_same(device_graph(dev, fragments, aff, k), base)
    n_edges = len(base[0])
    tight = 1 << (n_edges - 1).bit_length()          # the smallest table that holds the edges
    assert tight < capacity_for(fragments.size)
    assert_same(device_graph(dev, fragments, aff, k, tight), base)
    assert_same(device_graph(dev, fragments, aff, k, 1 << 20), base)


# ---- 9. refusals, before anything is launched ------------------------------------------------------
def test_refusals(dev):
    lib = _native.lib()
    shape = (9, 10, 37)
    aff, fragments, k = random_case(shape)
    call = Call(dev, fragments, aff, k, 4096)

    def refused(code, what, **changes):
        args = call.args()
        names = ["labels", "aff", "dtype", "dims", "n_labels", "capacity", "edges", "counts", "sums", "sizes",
                 "state", "ws", "need", "stream"]
        for name, value in changes.items():
            args[names.index(name)] = value
        assert call.run(args) == code, (changes, _native.last_error())
        assert what in _native.last_error(), (changes, _native.last_error())
        assert call.untouched(), changes

    for name in ("labels", "aff", "edges", "counts", "sums", "sizes", "state", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "aff_dtype", dtype=2)
    refused(-1, "aff_dtype", dtype=-1)
    refused(-1, "dims", dims=_native.int3((9, 0, 37)))
    refused(-1, "dims", dims=_native.int3((9, -10, 37)))
    refused(-1, "dims", dims=_native.int3((2048, 1024, 1024)))       # 2^31 voxels
    refused(-1, "n_labels", n_labels=-1)
    for capacity in (0, -4096, 4095, 3 << 10, (1 << 30) + 1, 1 << 31):
        refused(-1, "edge_capacity", capacity=capacity)
        assert lib.exaspim_region_graph_workspace_bytes(call.dims, k, capacity) == 0
        assert "edge_capacity" in _native.last_error()
    refused(-1, "misaligned", labels=call.labels.data_ptr() + 2)
    refused(-1, "misaligned", aff=call.aff.data_ptr() + 2)
    refused(-1, "misaligned", edges=call.edges.data_ptr() + 2)
    refused(-1, "misaligned", counts=call.counts.data_ptr() + 4)
    refused(-1, "misaligned", sums=call.sums.data_ptr() + 4)
    refused(-1, "misaligned", sizes=call.sizes.data_ptr() + 4)
    refused(-1, "misaligned", state=call.state.data_ptr() + 2)
    refused(-1, "misaligned", ws=call.ws.data_ptr() + 8)
    refused(-3, "workspace", need=call.need - 1)
    assert lib.exaspim_region_graph_workspace_bytes(_native.int3((9, 0, 37)), k, 4096) == 0
    assert lib.exaspim_region_graph_workspace_bytes(_native.int3((2048, 1024, 1024)), k, 4096) == 0
    assert lib.exaspim_region_graph_workspace_bytes(call.dims, -1, 4096) == 0
    half = Call(dev, fragments, aff.astype(np.float16), k, 4096)
    args = half.args()
    args[1] = half.aff.data_ptr() + 1
    assert half.run(args) == -1 and "misaligned" in _native.last_error() and half.untouched()
    # and the same buffers do serve a sound call afterwards
    assert call.run() == 0, _native.last_error()
    assert_same(call.result()[0], region_graph_ref.region_graph(fragments, aff, k))


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, fragments, _ = random_case((9, 10, 37))
    with pytest.raises(ValueError, match="edge_capacity"):
        inference.region_graph(fragments, aff, edge_capacity=1000)
    with pytest.raises(ValueError, match="affinities must be"):
        inference.region_graph(fragments, aff[0])
    with pytest.raises(TypeError):
        inference.region_graph(fragments.astype(np.int64), aff)
    with pytest.raises(ValueError, match="no affinities to score"):
        inference.agglomerate_affinities(torch.from_numpy(aff[0].copy()).to(dev))
    with pytest.raises(ValueError, match="non-decreasing"):
        inference.agglomerate_affinities(torch.from_numpy(aff.copy()).to(dev), [0.9, 0.8])


# ---- 10. the public region_graph -------------------------------------------------------------------
def test_public_region_graph_takes_numpy_and_device_tensors(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, fragments, k = random_case((17, 8, 33))
    want = region_graph_ref.region_graph(fragments, aff, k)
    assert_same(inference.region_graph(fragments, aff), want)
    got = inference.region_graph(torch.from_numpy(fragments.copy()).to(dev), torch.from_numpy(aff.copy()).to(dev),
                                 edge_capacity=1 << 14)
    assert_same(got, want)


# ---- 11. the table look-up -------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(4099, 0), (4099, 1), (3, 0)])
def test_apply_label_table_with_out_of_range_labels(dev, n, offset):
    lib = _native.lib()
    rng = np.random.default_rng(41)
    table = rng.integers(0, 1000, 50).astype(np.int32)
    labels = rng.integers(-5, 60, n).astype(np.int32)
    labels[:3] = [np.iinfo(np.int32).max, np.iinfo(np.int32).min, 50]
    want = np.where((labels >= 0) & (labels < 50), table[np.clip(labels, 0, 49)], 0).astype(np.int32)
    buf = torch.full((offset + n + GUARD,), -1234567, dtype=torch.int32, device=dev)
    buf[offset:offset + n] = torch.from_numpy(labels).to(dev)
    tab = torch.from_numpy(table).to(dev)
    rc = lib.exaspim_apply_label_table(buf.data_ptr() + 4 * offset, n, tab.data_ptr(), 50, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    np.testing.assert_array_equal(buf[offset:offset + n].cpu().numpy(), want)
    assert (buf[:offset] == -1234567).all() and (buf[offset + n:] == -1234567).all()
    assert lib.exaspim_apply_label_table(None, n, tab.data_ptr(), 50, None) == -1
    assert lib.exaspim_apply_label_table(buf.data_ptr(), n, None, 50, None) == -1
    assert lib.exaspim_apply_label_table(buf.data_ptr(), n, tab.data_ptr(), 0, None) == -1
    assert lib.exaspim_apply_label_table(buf.data_ptr() + 2, n, tab.data_ptr(), 50, None) == -1
    assert lib.exaspim_apply_label_table(buf.data_ptr(), 0, tab.data_ptr(), 50, None) == 0


# ---- 12. agglomerate_affinities end to end ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 10, 37), (17, 8, 33)])
def test_agglomerate_affinities_on_random_affinities(dev, shape):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = random_case(shape)[0]
    t = torch.from_numpy(aff.copy()).to(dev)
    partly = False
    for thresholds, min_size in (([0.55], 0), ([0.5, 0.6], 0), ([0.6], 10), ([0.9], 0)):
        want = region_graph_ref.agglomerate_affinities(aff, thresholds, min_size, 0.75)
        got = inference.agglomerate_affinities(t, thresholds, min_size, fragment_threshold=0.75,
                                               return_device_tensor=True)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device.type == "cuda"
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        partly = partly or 1 < int(want.max()) < random_case(shape)[2]
    assert partly
    half = aff.astype(np.float16)
    want = region_graph_ref.agglomerate_affinities(half, [0.6], 5, 0.75)
    np.testing.assert_array_equal(inference.agglomerate_affinities(half, [0.6], 5, fragment_threshold=0.75), want)


def test_agglomerate_affinities_numpy_in_numpy_out_with_the_defaults(dev, golden):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = golden("g10_components.npz")["aff"].astype(np.float32)
    fragments, k = components_ref.components(aff, 0.5, 0)
    assert k <= 64                     # keeps the naive oracle quick
    want = region_graph_ref.agglomerate_affinities(aff)
    got = inference.agglomerate_affinities(aff)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, want)


def test_predict_device_tensor_feeds_agglomeration(dev):
    from aind_exaspim_neuron_segmentation_amd import inference
    from aind_exaspim_neuron_segmentation_amd.machine_learning.unet3d import UNet3D

    sd = synthetic.synth_state_dict(3, 0.125, seed=1)
    model = UNet3D(output_channels=3, width_multiplier=0.125)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to(dev).eval()
    vol = synthetic.synth_volume((40, 48, 56), seed=21)
    pred = inference.predict(vol, model, batch_size=3, patch_shape=(32, 32, 32), overlap=(8, 8, 8), trim=4,
                             verbose=False, return_device_tensor=True)
    assert pred.device.type == "cuda" and pred.dtype == torch.float32 and tuple(pred.shape) == (3, 40, 48, 56)
    host = pred.cpu().numpy()
    # this model's outputs lie in a narrow band: fragments at its 0.6 quantile (some 160 of them, which
    # keeps the naive oracle quick), merged where a contact's mean is above the median contact's
    fragment_threshold = float(np.quantile(host[:, 4:-4, 4:-4, 4:-4], 0.6))
    fragments, k = components_ref.components(host, fragment_threshold, 0)
    edges, counts, sums, sizes = region_graph_ref.region_graph(fragments, host, k)
    assert 2 <= k <= 2000 and 1 <= len(edges) <= 5000
    assert_same(inference.region_graph(fragments, pred), (edges, counts, sums, sizes))
    means = np.sort(sums.astype(np.float64) / counts / ONE)
    threshold = 1.0 - float(means[len(means) // 2])
    for min_size in (0, 20):
        table, s = region_graph_ref.agglomerate(edges, counts, sums, sizes, threshold, min_size)
        if min_size == 0:
            assert 1 <= s < k
        got = inference.agglomerate_affinities(pred, [threshold], min_size, fragment_threshold=fragment_threshold,
                                               return_device_tensor=True)
        np.testing.assert_array_equal(got.cpu().numpy(), table[fragments])
        assert int(got.max()) == s


# ---- 13. end to end at 10^4 fragments, against the heap oracle ------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_watershed_fragments_at_sixteen_thousand(dev, dtype):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, fragments, k, graph = region_graph_ref.fragment_volume("watershed", dtype)
    assert aff.dtype == dtype and k >= 10000
    aff = np.array(aff)                         # the shared one is read-only
    for threshold in (0.6, 0.7):
        table, s = region_graph_ref.agglomerate_fast(*graph, threshold, 0)
        assert 1 < s < k
        got = inference.agglomerate_affinities(aff, [threshold], 0, fragments="watershed", aff_threshold_low=0.3,
                                               aff_threshold_high=0.7)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, table[fragments])


def test_component_fragments_at_twenty_seven_thousand_whole_and_in_slabs(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, fragments, k, graph = region_graph_ref.fragment_volume("components")
    table, s = region_graph_ref.agglomerate_fast(*graph, 0.6, 10)
    assert k >= 10000 and len(graph[0]) >= 3 * k and 1 < s < k
    want = table[fragments]
    aff = np.array(aff)                         # the shared one is read-only
    whole = inference.agglomerate_affinities(aff, [0.6], 10, fragment_threshold=0.75)
    np.testing.assert_array_equal(whole, want)
    for slab_depth in (1, 8, 13):               # 33 planes: one-plane slabs, 4 x 8 + 1, 13 + 13 + 7
        got = inference.agglomerate_affinities_streaming(aff, [0.6], 10, fragment_threshold=0.75,
                                                         slab_depth=slab_depth)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, whole, err_msg=f"slab_depth {slab_depth}")


# ---- 14. more tiles than one capped launch covers ---------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_grid_stride_over_tiles(dev, dtype):
    """
    tile_graph launches at most 65536 workgroups of one tile each and strides beyond that; its LDS table is
    cleared once and left empty by every flush. (589824, 9, 2) has 147 456 tiles: every workgroup makes two
    or three trips, and what the planes behind the first 65536 tiles add has edges of its own with more than
    one voxel edge each. The table has four slots per edge of the oracle: six per voxel, as capacity_for
    sizes it, would be 2^26 slots.
    """
    labels, aff, k, want, behind = region_graph_ref.stride_volume(dtype)
    shape = labels.shape
    assert aff.dtype == dtype
    assert -(-shape[0] // TILE[0]) * -(-shape[1] // TILE[1]) * -(-shape[2] // TILE[2]) >= 2 * 65536
    assert len(behind[0]) >= 1000 and int(behind[1].max()) >= 2
    capacity = 1 << (4 * len(want[0]) - 1).bit_length()
    assert_same(device_graph(dev, labels, aff, k, capacity), want)      # asserts the guards and the overflow flag
