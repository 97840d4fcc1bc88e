"""
exaspim_components / inference.affinities_to_components on the GPU (-m gpu), bit for bit against
the CPU oracle (tests/components_ref.py): the reference's own affinities (golden g10), random
affinities around bond percolation, a serpentine (the longest parent chain a volume admits),
degenerate shapes, the edge convention, the threshold rule, float16 input, foreground mode,
determinism and memory discipline, a long thin volume with more voxels and more tiles than one
launch covers (in foreground mode and, with affinities derived from the same foreground, in affinity
mode), and predict() feeding it on the device.

The kernels merge 8 x 8 x 32 tiles in LDS and then across tile faces; the random cases assert from
the oracle that components cross tile faces. "One larger than a tile" is held as a voxel count
(> 2048) at thresholds 0.6 and 0.75; at 0.8 the largest component of such a volume has about 200
voxels, fewer than any useful tile, so there the assertion is that a component occupies more than
one tile, which is asserted at the other thresholds as well.
"""

import numpy as np
import pytest
import torch

import components_ref
from aind_exaspim_neuron_segmentation_amd import _native
from aind_exaspim_neuron_segmentation_amd.utils import synthetic

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)
TILE_VOXELS = 8 * 8 * 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def run(dev, aff, threshold, min_size):
    """(labels, K) from the device for a numpy or torch input."""
    from aind_exaspim_neuron_segmentation_amd import inference

    t = torch.from_numpy(np.array(aff, order="C")).to(dev) if isinstance(aff, np.ndarray) else aff
    labels, count = inference._components_on_device(t, threshold, min_size)
    return labels.cpu().numpy(), int(count.cpu()[0])


def check(dev, aff, threshold, min_size):
    want, k = components_ref.components(aff, threshold, min_size)
    got, got_k = run(dev, aff, threshold, min_size)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert got_k == k == int(got.max(initial=0))
    np.testing.assert_array_equal(got, want)
    return want, k


# ---- 1. the reference's affinities -------------------------------------------------------------
@pytest.fixture(scope="module")
def g10(golden):
    g = golden("g10_components.npz")
    return g["aff"].astype(np.float32), g["labels"]


@pytest.mark.parametrize("min_size,k", [(0, 7), (25, 6), (100, 4), (2804, 0)])
def test_g10_equals_oracle_and_reference_partition(dev, g10, min_size, k):
    aff, labels = g10
    want, got_k = check(dev, aff, 0.5, min_size)
    assert got_k == k
    if min_size == 0:
        got, _ = run(dev, aff, 0.5, 0)
        assert components_ref.same_partition(got, labels)


def test_g10_through_the_public_function(dev, g10):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff, _ = g10
    want, _ = components_ref.components(aff, 0.5, 100)
    got = inference.affinities_to_components(aff)          # numpy in, numpy out, the defaults
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    t = inference.affinities_to_components(torch.from_numpy(aff).to(dev), return_device_tensor=True)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device.type == "cuda"
    np.testing.assert_array_equal(t.cpu().numpy(), want)


# ---- 2. random affinities near bond percolation --------------------------------------------------
_RANDOM = {}


def random_affinities(shape):
    if shape not in _RANDOM:
        a = np.random.default_rng(5).random((3,) + shape).astype(np.float32)
        a.setflags(write=False)
        _RANDOM[shape] = a
    return _RANDOM[shape]


def tiles_per_component(labels):
    """Number of distinct tiles every component 1 .. K occupies."""
    z, y, x = np.nonzero(labels)
    tile = ((z // TILE[0]) * 4096 + y // TILE[1]) * 4096 + x // TILE[2]
    pairs = np.unique(np.stack([labels[z, y, x].astype(np.int64), tile]), axis=1)
    return np.bincount(pairs[0])[1:]


@pytest.mark.parametrize("threshold", [0.6, 0.75, 0.8])
@pytest.mark.parametrize("shape", [(24, 40, 72), (23, 37, 71)])
def test_random_affinities_near_percolation(dev, shape, threshold):
    aff = random_affinities(shape)
    want, k = check(dev, aff, threshold, 0)
    sizes = np.bincount(want.ravel())[1:]
    assert k >= 2
    assert tiles_per_component(want).max() >= 2
    if threshold < 0.8:
        assert sizes.max() > TILE_VOXELS
    if shape == (24, 40, 72):   # the oracle itself, against figures worked out independently
        assert (k, int(sizes.max())) == {0.6: (937, 62976), 0.75: (7134, 4367), 0.8: (10468, 221)}[threshold]
    check(dev, aff, threshold, 100)


# ---- 3. a serpentine -----------------------------------------------------------------------------
def serpentine(shape):
    """Affinities that switch on one boustrophedon path through every voxel."""
    d, h, w = shape
    path = []
    row = 0
    for z in range(d):
        for y in (range(h) if z % 2 == 0 else range(h - 1, -1, -1)):
            for x in (range(w) if row % 2 == 0 else range(w - 1, -1, -1)):
                path.append((z, y, x))
            row += 1
    path = np.array(path)
    assert len(path) == d * h * w
    a, b = path[:-1], path[1:]
    step = b - a
    assert (np.abs(step).sum(axis=1) == 1).all()
    axis = np.abs(step).argmax(axis=1)
    low = np.minimum(a, b)
    aff = np.zeros((3,) + shape, np.float32)
    aff[axis, low[:, 0], low[:, 1], low[:, 2]] = 1.0
    return aff


def test_serpentine_is_one_component(dev):
    aff = serpentine((16, 24, 40))
    want, k = check(dev, aff, 0.5, 0)
    assert k == 1 and (want == 1).all()
    # cut in the middle: two components, numbered in raster order
    aff[2, 8, 0, 19] = 0.0
    want, k = check(dev, aff, 0.5, 0)
    assert k == 2


# ---- 4. degenerate shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 9), (1, 33, 65), (9, 1, 1)])
def test_degenerate_shapes(dev, shape):
    rng = np.random.default_rng(7)
    aff = rng.random((3,) + shape).astype(np.float32)
    check(dev, aff, 0.4, 0)
    check(dev, np.ones((3,) + shape, np.float32), 0.5, 0)
    want, k = check(dev, np.zeros((3,) + shape, np.float32), 0.5, 0)
    assert k == 0 and not want.any()


# ---- 5. entries that leave the volume ------------------------------------------------------------
def test_high_face_entries_are_ignored(dev):
    shape = (9, 17, 35)
    aff = np.random.default_rng(11).random((3,) + shape).astype(np.float32)
    base, k = run(dev, aff, 0.7, 0)
    hot = aff.copy()
    hot[0, -1] = hot[1, :, -1] = hot[2, :, :, -1] = 1.0
    got, got_k = run(dev, hot, 0.7, 0)
    np.testing.assert_array_equal(got, base)
    assert got_k == k
    check(dev, hot, 0.7, 0)


# ---- 6. the threshold ----------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.3, 0.5, 0.1])
def test_threshold_edge(dev, threshold):
    thr = np.float32(threshold)
    below = np.nextafter(thr, np.float32(0))
    assert below < thr
    aff = np.zeros((3, 4, 5, 12), np.float32)
    aff[2, 0, 0, 0:3] = thr        # on: 4 voxels
    aff[2, 1, 1, 0:3] = below      # off
    aff[2, 2, 2, 0:3] = np.nan     # off
    aff[1, 3, 0:2, 5] = thr        # on: 3 voxels along y
    aff[0, 0:2, 4, 8] = np.nan
    want, k = check(dev, aff, threshold, 0)
    assert k == 2 and (want == 1).sum() == 4 and (want == 2).sum() == 3
    check(dev, aff.astype(np.float16).astype(np.float32), threshold, 0)


# ---- 7. float16 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 20, 40), (7, 9, 13)])
def test_float16_equals_the_rounded_float32(dev, shape):
    half = np.random.default_rng(13).random((3,) + shape).astype(np.float16)
    got16, k16 = run(dev, half, 0.7, 2)
    got32, k32 = run(dev, half.astype(np.float32), 0.7, 2)
    np.testing.assert_array_equal(got16, got32)
    assert k16 == k32
    check(dev, half, 0.7, 2)
    fg = half[0]
    check(dev, fg, 0.6, 0)


# ---- 8. foreground mode --------------------------------------------------------------------------
def test_foreground_mode(dev):
    p = np.random.default_rng(17).random((13, 21, 45)).astype(np.float32)
    for thr in (0.55, 0.75):
        for min_size in (0, 1, 10):
            check(dev, p, thr, min_size)
    one = np.zeros((5, 9, 33), np.float32)
    one[2, 3, 31] = 0.9
    one[4, 8, 0:2] = 0.9
    want, k = check(dev, one, 0.5, 0)
    assert k == 2 and want[2, 3, 31] == 1
    want, k = check(dev, one, 0.5, 1)
    assert k == 1 and want[2, 3, 31] == 0 and want[4, 8, 0] == 1


# ---- 9. determinism and memory discipline --------------------------------------------------------
def test_determinism_guards_and_workspace_check(dev):
    shape = (24, 40, 72)
    aff = torch.from_numpy(random_affinities(shape).copy()).to(dev)
    n = int(np.prod(shape))
    lib = _native.lib()
    dims = _native.int3(shape)
    need = lib.exaspim_components_workspace_bytes(dims)
    assert need >= 5 * n
    guard = 64
    outs = []
    for _ in range(2):
        labels = torch.full((n + guard,), -1234567, dtype=torch.int32, device=dev)
        count = torch.full((1 + guard,), -7654321, dtype=torch.int32, device=dev)
        ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
        rc = lib.exaspim_components(aff.data_ptr(), _native.AFF_F32, 3, dims, 0.75, 0, labels.data_ptr(),
                                    count.data_ptr(), ws.data_ptr(), need, None)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        assert (labels[n:] == -1234567).all() and (count[1:] == -7654321).all()
        assert (ws[need:] == 0xA5).all()
        outs.append((labels[:n].cpu().numpy().tobytes(), int(count[0].cpu())))
    assert outs[0] == outs[1]
    want, k = components_ref.components(random_affinities(shape), 0.75, 0)
    assert outs[0] == (want.tobytes(), k)

    # one byte short: refused before anything is launched
    labels = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)
    rc = lib.exaspim_components(aff.data_ptr(), _native.AFF_F32, 3, dims, 0.75, 0, labels.data_ptr(),
                                count.data_ptr(), ws.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -3 and "workspace" in _native.last_error()
    assert (labels == -1234567).all() and int(count[0].cpu()) == -7654321 and (ws == 0xA5).all()


# ---- 9b. more voxels and more tiles than one launch covers ----------------------------------------
_STRIDE = []


def stride_case():
    """(on, labels, K): the foreground of the two stride tests and scipy.ndimage.label of it, computed once."""
    from scipy import ndimage

    if not _STRIDE:
        on = np.random.default_rng(23).random((262152, 9, 9), dtype=np.float32) >= np.float32(0.5)
        want, k = ndimage.label(on)
        want.setflags(write=False)      # on goes to the device through torch.from_numpy, which wants it writable
        _STRIDE.append((on, want, k))
    return _STRIDE[0]


def test_grid_stride_tails_against_ndimage_label(dev):
    """
    The per-voxel kernels launch at most 65536 workgroups of 256 threads and tile_pass at most 65536
    workgroups of one tile each; beyond that they stride. (262152, 9, 9) has 21.2M voxels (> 65536 *
    256 = 16.8M), 32769 * 2 * 1 = 65538 tiles and 10369 scan blocks (> 4096, so the middle pass of
    the prefix sum carries across chunks), which is the smallest shape that has all three: a tile
    that is mostly outside the volume costs no voxels. Foreground mode at p = 0.5 in a 9 x 9 column
    gives components that run through many tiles along z. scipy.ndimage.label numbers in raster
    order as well, so the arrays are compared as they are.
    """
    from aind_exaspim_neuron_segmentation_amd import inference

    on, want, k = stride_case()
    shape = on.shape
    assert np.prod(shape) > 65536 * 256
    assert -(-shape[0] // TILE[0]) * -(-shape[1] // TILE[1]) * -(-shape[2] // TILE[2]) > 65536
    assert k >= 2 and np.ptp(np.nonzero(want == np.bincount(want.ravel())[1:].argmax() + 1)[0]) >= 2 * TILE[0]
    got, count = inference._components_on_device(torch.from_numpy(on).to(dev).to(torch.float32), 0.5, 0)
    assert int(count.cpu()[0]) == k
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_grid_stride_tails_in_affinity_mode(dev):
    """
    The same volume through edge_mask_affinity (a width of 9 is its scalar form, one voxel per thread: more
    voxels than one capped launch covers): affinities that are on exactly between two on voxels of the
    foreground above. Their components are the foreground's without the lone voxels, which affinity mode
    never keeps, numbered in the same raster order (tests/test_components_cpu.py holds that identity to the
    oracle).
    """
    from aind_exaspim_neuron_segmentation_amd import inference

    on, labelled, n = stride_case()
    assert np.prod(on.shape) > 65536 * 256 and on.shape[2] % 4 != 0
    want, k = components_ref.drop_singletons(labelled, n)
    assert 2 <= k < n
    aff = torch.from_numpy(components_ref.affinities_of_foreground(on)).to(dev)
    got, count = inference._components_on_device(aff, 0.5, 0)
    assert int(count.cpu()[0]) == k
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ---- 10. predict() feeding it on the device --------------------------------------------------------
def test_predict_device_tensor_feeds_components(dev):
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
    covered = host[:, 4:-4, 4:-4, 4:-4]
    threshold = float(np.median(covered))
    for min_size in (0, 20):
        want, k = components_ref.components(host, threshold, min_size)
        if min_size == 0:
            assert k >= 2
        got = inference.affinities_to_components(pred, threshold, min_size, return_device_tensor=True)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert int(got.max()) == k
