"""
exaspim_watershed_fragments / inference.watershed_fragments / agglomerate_affinities(...,
fragments="watershed") on the GPU (-m gpu), label for label against the CPU oracle written from the
definition (tests/watershed_ref.py fragments(); tests/test_watershed_cpu.py holds that oracle to the
serial watershed): shapes around the 8 x 8 x 32 tile of the mask kernel, the scalar path (a width that
is no multiple of the vector, a base pointer off by one element), float16 input with tied values, the
hand-built lines along all three axes, more tiles than one capped launch covers (on the scalar and on the
vector path), memory discipline,
every refusal, the agglomeration end to end and predict() feeding it on the device.

The mask kernel decides an edge from the steepest edges of both of its ends and computes those of the
voxels one step beyond the tile's three high faces itself; the (17, 17, 65) cases assert from the
oracle that edges across tile faces are on through the choice of their upper end alone.
"""

import numpy as np
import pytest
import torch

import components_ref
import region_graph_ref
import watershed_ref
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic
from watershed_ref import LINES, random_affinities

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def run(dev, aff, low, high, min_size=0):
    """(labels, K) from the device for a numpy or torch input."""
    from aind_exaspim_neuron_segmentation_amd import inference

    t = torch.from_numpy(np.array(aff, order="C")).to(dev) if isinstance(aff, np.ndarray) else aff
    labels, count = inference._watershed_on_device(t, low, high, min_size)
    return labels.cpu().numpy(), int(count.cpu()[0])


def check(dev, aff, low, high, min_size=0):
    want, k = watershed_ref.fragments(aff, low, high, min_size)
    got, got_k = run(dev, aff, low, high, min_size)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert got_k == k == int(got.max(initial=0))
    np.testing.assert_array_equal(got, want)
    return want, k


# ---- 1. shapes around the tile -----------------------------------------------------------------------
INPUTS = [("uniform", 0.1, 0.9999), ("uniform", 0.3, 0.7), ("saturated", 0.3, 0.7)]
AROUND_THE_TILE = [(7, 5, 3), (8, 8, 32), (9, 9, 33), (16, 16, 64), (17, 17, 65), (1, 1, 40), (1, 40, 1), (40, 1, 1),
                   (3, 1, 5), (5, 6, 30), (9, 10, 36)]


@pytest.mark.parametrize("kind,low,high", INPUTS)
@pytest.mark.parametrize("shape", AROUND_THE_TILE)
def test_shapes_around_the_tile(dev, shape, kind, low, high):
    """(5, 6, 30): a width that is no multiple of 4, the scalar path; (9, 10, 36): the vector path with a
    last tile of 4 voxels along x."""
    aff = random_affinities(kind, shape)
    _, k = check(dev, aff, low, high)
    assert k >= 1
    check(dev, aff, low, high, 3)


def test_a_base_pointer_off_by_one_element_takes_the_scalar_path(dev):
    shape = (9, 10, 36)
    aff = random_affinities("uniform", shape)
    flat = torch.zeros(aff.size + 5, dtype=torch.float32, device=dev)
    for offset in (0, 1):
        view = flat[offset:offset + aff.size].view((3,) + shape)
        view.copy_(torch.from_numpy(aff.copy()))
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
        want, k = watershed_ref.fragments(aff, 0.3, 0.7, 0)
        got, got_k = run(dev, view, 0.3, 0.7)
        np.testing.assert_array_equal(got, want)
        assert got_k == k
    half = aff.astype(np.float16)
    flat16 = torch.zeros(aff.size + 9, dtype=torch.float16, device=dev)
    view = flat16[1:1 + aff.size].view((3,) + shape)
    view.copy_(torch.from_numpy(half))
    assert view.data_ptr() % 16 == 2
    want, k = watershed_ref.fragments(half, 0.3, 0.7, 0)
    got, got_k = run(dev, view, 0.3, 0.7)
    np.testing.assert_array_equal(got, want)
    assert got_k == k


# ---- 2. what the (17, 17, 65) cases exercise, by the oracle alone ------------------------------------
def on_through_the_upper_end_across_a_tile_face(aff, low, high):
    """Per axis: on edges with a < high that cross a tile face and are the steepest edge of their upper
    end but not of their lower end."""
    a = np.asarray(aff).astype(np.float32)
    code = watershed_ref.steepest(a, low)
    counts = []
    for axis in range(3):
        up = 1 + watershed_ref.DIRECTIONS.index((axis, +1))
        down = 1 + watershed_ref.DIRECTIONS.index((axis, -1))
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        v = a[axis][lo]
        m = (v > np.float32(low)) & (v < np.float32(high)) & (code[lo] != up) & (code[hi] == down)
        counts.append(int((np.nonzero(m)[axis] % TILE[axis] == TILE[axis] - 1).sum()))
    return counts


def tiles_per_fragment(labels):
    z, y, x = np.nonzero(labels)
    tile = ((z // TILE[0]) * 4096 + y // TILE[1]) * 4096 + x // TILE[2]
    pairs = np.unique(np.stack([labels[z, y, x].astype(np.int64), tile]), axis=1)
    return np.bincount(pairs[0])[1:]


# uniform values at low = 0.1 leave a voxel without an eligible edge with probability 1e-6 .. 1e-3
# (six edges inside, three at a corner): seed 21 is the first from 7 on whose volume has one
@pytest.mark.parametrize("kind,low,high,seed", [("uniform", 0.1, 0.9999, 21), ("uniform", 0.3, 0.7, 7),
                                                ("saturated", 0.3, 0.7, 7)])
def test_halo_tiles_and_background_are_exercised(dev, kind, low, high, seed):
    shape = (17, 17, 65)
    aff = random_affinities(kind, shape, seed)
    want, k = watershed_ref.fragments(aff, low, high, 0)
    assert min(on_through_the_upper_end_across_a_tile_face(aff, low, high)) >= 1
    assert tiles_per_fragment(want).max() >= 2
    assert (want == 0).any() and k >= 2
    if kind == "saturated":      # few large basins: the largest spreads over most of the 27 tiles
        assert k < 200 and np.bincount(want.ravel())[1:].max() > 8 * 8 * 32
    check(dev, aff, low, high)


# ---- 3. float16 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 17, 65), (9, 10, 36), (8, 8, 32)])
def test_float16_input_with_tied_values(dev, shape):
    """Half precision has 2^-11 steps below 1: some voxels get two equal maximal edges, which pins the tie
    order on the device. (9, 10, 36): a width that is a multiple of 4 but not of 8, the scalar path."""
    half = random_affinities("uniform", shape).astype(np.float16)
    if shape == (17, 17, 65):
        assert watershed_ref.tied_voxels(half, 0.1, 0.9999) >= 10
    for low, high in ((0.1, 0.9999), (0.3, 0.7)):
        want, k = check(dev, half, low, high)
        got32, k32 = run(dev, half.astype(np.float32), low, high)
        np.testing.assert_array_equal(got32, want)
        assert k32 == k


def test_quantised_values_tie_everywhere(dev):
    aff = (np.floor(random_affinities("uniform", (17, 17, 65)) * 8) / 8).astype(np.float32)
    assert watershed_ref.tied_voxels(aff, 0.1, 0.9999) > 1000
    check(dev, aff, 0.1, 0.9999)
    check(dev, aff.astype(np.float16), 0.1, 0.9999)


# ---- 4. the hand-built lines ---------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_hand_built_lines(dev, axis):
    for name, values, low, high, min_size, labels in LINES:
        aff = watershed_ref.line_affinities(axis, values)
        got, k = run(dev, aff, low, high, min_size)
        assert got.ravel().tolist() == labels, name
        assert k == max(labels), name


def test_high_face_entries_are_ignored(dev):
    shape = (9, 17, 36)
    aff = random_affinities("uniform", shape).copy()
    base, k = run(dev, aff, 0.3, 0.7)
    for hot in (1.0, np.inf, np.nan):
        aff[0, -1] = aff[1, :, -1] = aff[2, :, :, -1] = hot
        got, got_k = run(dev, aff, 0.3, 0.7)
        np.testing.assert_array_equal(got, base)
        assert got_k == k
    check(dev, aff, 0.3, 0.7)


def test_no_relation_between_low_and_high_is_required(dev):
    aff = random_affinities("uniform", (9, 9, 33))
    want, k = check(dev, aff, 0.6, 0.2)          # every eligible edge is on: components above 0.6
    above = np.nextafter(np.float32(0.6), np.float32(1))
    np.testing.assert_array_equal(want, components_ref.components(aff, above, 0)[0])
    check(dev, aff, 0.5, 0.5)


# ---- 5. more tiles than one capped launch covers ---------------------------------------------------------
@pytest.mark.parametrize("shape", [(262152, 9, 9), (262160, 9, 4)], ids=["scalar", "vector"])
def test_grid_stride_over_tiles(dev, shape):
    """
    The mask kernel launches at most 65536 workgroups of one tile each and strides beyond that;
    (262152, 9, 9), the shape tests/test_gpu_components.py uses for the same purpose, has 65538 tiles
    (and more voxels and scan blocks than one launch of the later passes covers). A width of 9 is the
    scalar path; every tile has voxels beyond the volume in y and x. (262160, 9, 4) has 65540 tiles and a
    width of one vector: the four-voxel path, whose second trip starts from the remapped tile of the first.
    """
    assert -(-shape[0] // TILE[0]) * -(-shape[1] // TILE[1]) * -(-shape[2] // TILE[2]) > 65536
    assert (shape[2] % 4 == 0) == (shape == (262160, 9, 4))
    aff = np.random.default_rng(23).random((3,) + shape, dtype=np.float32)
    want, k = watershed_ref.fragments(aff, 0.3, 0.7, 0)
    assert k >= 2 and tiles_per_fragment(want[-64:]).max() >= 2
    got, got_k = run(dev, aff, 0.3, 0.7)
    assert got_k == k
    np.testing.assert_array_equal(got, want)


# ---- 6. determinism and memory discipline ----------------------------------------------------------------
def test_determinism_guards_and_workspace_check(dev):
    shape = (17, 17, 65)
    host = random_affinities("saturated", shape)
    aff = torch.from_numpy(host.copy()).to(dev)
    n = int(np.prod(shape))
    lib = _native.lib()
    dims = _native.int3(shape)
    need = lib.exaspim_watershed_workspace_bytes(dims)
    assert need >= 5 * n and need == lib.exaspim_components_workspace_bytes(dims)
    guard = 64
    outs = []
    for _ in range(2):
        labels = torch.full((n + guard,), -1234567, dtype=torch.int32, device=dev)
        count = torch.full((1 + guard,), -7654321, dtype=torch.int32, device=dev)
        ws = torch.full((need + guard,), 0xFF, dtype=torch.uint8, device=dev)
        rc = lib.exaspim_watershed_fragments(aff.data_ptr(), _native.AFF_F32, dims, 0.3, 0.7, 0, labels.data_ptr(),
                                             count.data_ptr(), ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        assert (labels[n:] == -1234567).all() and (count[1:] == -7654321).all()
        assert (ws[need:] == 0xFF).all()
        outs.append((labels[:n].cpu().numpy().tobytes(), int(count[0].cpu())))
    assert outs[0] == outs[1]
    want, k = watershed_ref.fragments(host, 0.3, 0.7, 0)
    assert outs[0] == (want.tobytes(), k)
    np.testing.assert_array_equal(aff.cpu().numpy(), host)          # the input is only read

    # one byte short: refused before anything is launched
    labels = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    rc = lib.exaspim_watershed_fragments(aff.data_ptr(), _native.AFF_F32, dims, 0.3, 0.7, 0, labels.data_ptr(),
                                         count.data_ptr(), ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -3 and "workspace" in _native.last_error()
    assert (labels == -1234567).all() and int(count[0].cpu()) == -7654321 and (ws == 0xFF).all()


# ---- 7. refusals, before anything is launched ------------------------------------------------------------
def test_refusals(dev):
    lib = _native.lib()
    shape = (9, 10, 36)
    host = random_affinities("uniform", shape)
    n = int(np.prod(shape))
    aff = torch.from_numpy(host.copy()).to(dev)
    half = torch.from_numpy(host.astype(np.float16)).to(dev)
    need = lib.exaspim_watershed_workspace_bytes(_native.int3(shape))
    labels = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    names = ["aff", "dtype", "dims", "low", "high", "min_size", "labels", "count", "ws", "need", "stream"]

    def call(**changes):
        args = [aff.data_ptr(), _native.AFF_F32, _native.int3(shape), 0.3, 0.7, 0, labels.data_ptr(),
                count.data_ptr(), ws.data_ptr(), need, None]
        for name, value in changes.items():
            args[names.index(name)] = value
        rc = lib.exaspim_watershed_fragments(*args)
        torch.cuda.synchronize()
        return rc

    def refused(code, what, **changes):
        assert call(**changes) == code, (changes, _native.last_error())
        assert what in _native.last_error(), (changes, _native.last_error())
        assert (labels == -1234567).all() and int(count[0].cpu()) == -7654321 and (ws == 0xFF).all(), changes

    for name in ("aff", "labels", "count", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "aff_dtype", dtype=2)
    refused(-1, "aff_dtype", dtype=-1)
    refused(-1, "dims", dims=_native.int3((9, 0, 36)))
    refused(-1, "dims", dims=_native.int3((9, -10, 36)))
    refused(-1, "dims", dims=_native.int3((2048, 1024, 1024)))       # 2^31 voxels
    refused(-1, "NaN", low=float("nan"))
    refused(-1, "NaN", high=float("nan"))
    refused(-1, "misaligned", aff=aff.data_ptr() + 2)
    refused(-1, "misaligned", aff=half.data_ptr() + 1, dtype=_native.AFF_F16)
    refused(-1, "misaligned", labels=labels.data_ptr() + 2)
    refused(-1, "misaligned", ws=ws.data_ptr() + 8)
    refused(-3, "workspace", need=need - 1)
    refused(-3, "workspace", need=0)
    assert lib.exaspim_watershed_workspace_bytes(_native.int3((9, 0, 36))) == 0
    assert "dims" in _native.last_error()
    assert lib.exaspim_watershed_workspace_bytes(_native.int3((2048, 1024, 1024))) == 0
    # and the same buffers do serve a sound call afterwards, infinite thresholds included
    assert call() == 0, _native.last_error()
    want, k = watershed_ref.fragments(host, 0.3, 0.7, 0)
    np.testing.assert_array_equal(labels.cpu().numpy().reshape(shape), want)
    assert int(count[0].cpu()) == k
    assert call(low=float("-inf"), high=float("inf")) == 0, _native.last_error()
    want, k = watershed_ref.fragments(host, -np.inf, np.inf, 0)
    np.testing.assert_array_equal(labels.cpu().numpy().reshape(shape), want)
    assert int(count[0].cpu()) == k


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = random_affinities("uniform", (9, 10, 36))
    t = torch.from_numpy(aff.copy()).to(dev)
    for bad in (aff[0], t[0], aff[:2], t[:, 0]):
        with pytest.raises(ValueError, match=r"\(3, D, H, W\)"):
            inference.watershed_fragments(bad)
    with pytest.raises(ValueError, match="no affinities"):
        inference.watershed_fragments(t[0])
    with pytest.raises(TypeError, match="float32 or float16"):
        inference.watershed_fragments(aff.astype(np.float64))
    with pytest.raises(TypeError, match="float32 or float16"):
        inference.watershed_fragments(t.double())
    with pytest.raises(TypeError):
        inference.watershed_fragments(aff.tolist())
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.watershed_fragments(torch.from_numpy(aff.copy()))
    with pytest.raises(ValueError, match="NaN"):
        inference.watershed_fragments(t, float("nan"), 0.9)
    with pytest.raises(ValueError, match="NaN"):
        inference.watershed_fragments(t, 0.1, float("nan"))
    with pytest.raises(ValueError, match="basins"):
        inference.agglomerate_affinities(t, fragments="basins")
    with pytest.raises(ValueError, match="NaN"):
        inference.agglomerate_affinities(t, fragments="watershed", aff_threshold_low=float("nan"))
    with pytest.raises(ValueError, match="no affinities to score"):
        inference.agglomerate_affinities(t[0], fragments="watershed")


def test_public_function_takes_numpy_and_device_tensors(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = random_affinities("saturated", (9, 9, 33))
    want, k = watershed_ref.fragments(aff, 0.1, 0.9999, 0)
    got = inference.watershed_fragments(aff)                       # numpy in, numpy out, the defaults
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    t = inference.watershed_fragments(torch.from_numpy(aff.copy()).to(dev), 0.3, 0.7, 4, return_device_tensor=True)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device.type == "cuda"
    np.testing.assert_array_equal(t.cpu().numpy(), watershed_ref.fragments(aff, 0.3, 0.7, 4)[0])


# ---- 8. the agglomeration end to end ---------------------------------------------------------------------
def watershed_chain(aff, threshold, min_size, low, high):
    """The oracle chain: fragments, region graph, naive agglomeration, size filter."""
    fragments, k = watershed_ref.fragments(aff, low, high, 0)
    edges, counts, sums, sizes = region_graph_ref.region_graph(fragments, aff, k)
    table, s = region_graph_ref.agglomerate(edges, counts, sums, sizes, threshold, min_size)
    return table[fragments], s, k


def test_agglomerate_affinities_with_watershed_fragments(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = random_affinities("saturated", (17, 17, 65))
    t = torch.from_numpy(aff.copy()).to(dev)
    want, s, k = watershed_chain(aff, 0.6, 0, 0.3, 0.7)
    assert k <= 200                                                 # keeps the naive oracle quick
    assert 1 < s < k
    got = inference.agglomerate_affinities(t, [0.5, 0.6], 0, fragments="watershed", aff_threshold_low=0.3,
                                           aff_threshold_high=0.7, return_device_tensor=True)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device.type == "cuda"
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert int(got.max()) == s
    want, s_filtered, _ = watershed_chain(aff, 0.6, 10, 0.3, 0.7)
    assert 1 <= s_filtered < s
    got = inference.agglomerate_affinities(aff, [0.6], 10, fragments="watershed", aff_threshold_low=0.3,
                                           aff_threshold_high=0.7)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    # fragment_threshold plays no part with watershed fragments
    again = inference.agglomerate_affinities(aff, [0.6], 10, fragments="watershed", aff_threshold_low=0.3,
                                             aff_threshold_high=0.7, fragment_threshold=0.99)
    np.testing.assert_array_equal(again, want)
    # and the defaults (0.1, 0.9999) on a volume small enough for the naive oracle
    small = random_affinities("saturated", (7, 5, 3))
    want, s, k = watershed_chain(small, 0.9, 2, 0.1, 0.9999)
    np.testing.assert_array_equal(inference.agglomerate_affinities(small, min_segment_size=2, fragments="watershed"),
                                  want)


def test_agglomerate_affinities_without_the_keyword_is_unchanged(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = random_affinities("uniform", (9, 10, 37))
    t = torch.from_numpy(aff.copy()).to(dev)
    for thresholds, min_size in (([0.55], 0), ([0.6], 10)):
        want = region_graph_ref.agglomerate_affinities(aff, thresholds, min_size, 0.75)
        got = inference.agglomerate_affinities(t, thresholds, min_size, fragment_threshold=0.75)
        np.testing.assert_array_equal(got, want)
        named = inference.agglomerate_affinities(t, thresholds, min_size, fragment_threshold=0.75,
                                                 fragments="components", aff_threshold_low=0.7,
                                                 aff_threshold_high=0.71)
        np.testing.assert_array_equal(named, want)
    assert 1 < int(want.max())


# ---- 9. predict() feeding it on the device ---------------------------------------------------------------
def test_predict_device_tensor_feeds_the_watershed(dev):
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
    # this model's outputs lie in a narrow band: thresholds from its own quantiles
    covered = host[:, 4:-4, 4:-4, 4:-4]
    low, high = float(np.quantile(covered, 0.3)), float(np.quantile(covered, 0.9))
    for min_size in (0, 20):
        want, k = watershed_ref.fragments(host, low, high, min_size)
        if min_size == 0:
            assert k >= 2
        got = inference.watershed_fragments(pred, low, high, min_size, return_device_tensor=True)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert int(got.max()) == k
