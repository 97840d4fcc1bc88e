"""
CPU-only checks around exaspim_components: the oracle the GPU tests hold the kernels to
(tests/components_ref.py) against the reference's own label mask and affinities (golden g10,
img_util.get_affinity_channels) and against scipy.ndimage.label, the affinity-mode case derived from a
foreground (affinities_of_foreground, drop_singletons), and the host side of
inference.affinities_to_components.
"""

import numpy as np
import pytest
from scipy import ndimage

import components_ref
from aind_exaspim_neuron_segmentation_amd import _native


@pytest.fixture(scope="module")
def g10(golden):
    g = golden("g10_components.npz")
    return g["aff"].astype(np.float32), g["labels"]


def test_fixture_is_what_the_tests_assume(g10):
    aff, labels = g10
    assert aff.shape == (3, 40, 70, 100) and labels.shape == (40, 70, 100) and labels.dtype == np.int32
    sizes = np.bincount(labels.ravel())[1:]
    assert sizes.size == 7 and sizes.min() == 25 and sizes.max() == 2804
    assert int((sizes > 100).sum()) == 4 and not (sizes == 1).any()


def test_oracle_recovers_the_reference_partition(g10):
    aff, labels = g10
    got, k = components_ref.components(aff, 0.5, 0)
    assert k == 7 == got.max() and got.dtype == np.int32
    assert components_ref.same_partition(got, labels)
    # scipy.ndimage.label numbers in raster order too: here even the ids agree
    np.testing.assert_array_equal(got, labels)
    got100, k100 = components_ref.components(aff, 0.5, 100)
    assert k100 == 4 == got100.max()
    # strict ">": 25 and 2804 are actual sizes
    assert components_ref.components(aff, 0.5, 24)[1] == 7
    assert components_ref.components(aff, 0.5, 25)[1] == 6
    assert components_ref.components(aff, 0.5, 2803)[1] == 1
    assert components_ref.components(aff, 0.5, 2804)[1] == 0


def test_affinities_of_a_foreground_give_its_components_without_lone_voxels():
    """The identity behind tests/test_gpu_components.py's stride test of affinity mode, on a thin column."""
    on = np.random.default_rng(23).random((20, 9, 9), dtype=np.float32) >= np.float32(0.5)
    aff = components_ref.affinities_of_foreground(on)
    assert aff.dtype == np.float32 and aff.shape == (3, 20, 9, 9)
    assert not aff[0, -1].any() and not aff[1, :, -1].any() and not aff[2, :, :, -1].any()
    assert aff[0, :-1].any() and aff[1, :, :-1].any() and aff[2, :, :, :-1].any()
    labelled, n = ndimage.label(on)
    want, k = components_ref.drop_singletons(labelled, n)
    lone = int((np.bincount(labelled.ravel())[1:] == 1).sum())
    assert lone >= 5 and k == n - lone and want.dtype == np.int32
    for threshold in (0.5, 1.0):
        got, got_k = components_ref.components(aff, threshold, 0)
        assert got_k == k
        np.testing.assert_array_equal(got, want)
    assert not np.array_equal(want, labelled)      # ids move down, they do not just vanish


def test_oracle_foreground_mode_is_ndimage_label():
    rng = np.random.default_rng(2)
    p = rng.random((11, 19, 23)).astype(np.float32)
    for thr in (0.5, 0.7):
        want, n = ndimage.label(p >= np.float32(thr))
        got, k = components_ref.components(p, thr, 0)
        assert k == n
        np.testing.assert_array_equal(got, want.astype(np.int32))
    # a lone on voxel: kept at 0, dropped at 1
    one = np.zeros((3, 4, 5), np.float32)
    one[1, 2, 3] = 1
    assert components_ref.components(one, 0.5, 0)[1] == 1
    assert components_ref.components(one, 0.5, 1)[1] == 0


def test_oracle_edge_rules():
    thr = np.float32(0.3)
    below = np.nextafter(thr, np.float32(0))
    aff = np.zeros((3, 2, 2, 4), np.float32)
    aff[2, 0, 0, 0] = thr       # on
    aff[2, 1, 1, 0] = below     # off
    aff[2, 0, 1, 1] = np.nan    # off
    aff[0, 1] = aff[1, :, 1] = aff[2, :, :, 3] = 1.0   # leave the volume
    got, k = components_ref.components(aff, 0.3, 0)
    want = np.zeros((2, 2, 4), np.int32)
    want[0, 0, :2] = 1
    assert k == 1
    np.testing.assert_array_equal(got, want)


def test_affinities_to_components_rejects_what_it_documents():
    import torch

    from aind_exaspim_neuron_segmentation_amd import inference

    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.affinities_to_components(torch.zeros(3, 4, 4, 4))
    with pytest.raises(TypeError):
        inference.affinities_to_components(np.zeros((3, 4, 4, 4), np.int32))
    with pytest.raises(TypeError):
        inference.affinities_to_components(torch.zeros(3, 4, 4, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        inference.affinities_to_components(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        inference.affinities_to_components(torch.zeros(2, 4, 4, 4))
    doc = inference.affinities_to_components.__doc__
    assert "waterz" in doc and "not" in doc


def test_components_entry_points_are_bound():
    assert "exaspim_components" in _native.SIGNATURES
    assert "exaspim_components_workspace_bytes" in _native.SIGNATURES
    assert (_native.AFF_F32, _native.AFF_F16) == (0, 1)


def test_components_argument_checks_need_no_device():
    """Shapes, dtypes, NULL pointers and the workspace size are checked before anything is launched.

    Every call passes workspace_bytes = 0, which no volume accepts: should the check a line is
    about ever regress, the call still ends with EXASPIM_E_WORKSPACE instead of a launch on the
    made-up addresses.
    """
    import __graft_entry__  # noqa: F401  (repository root on sys.path)
    import os

    if not os.path.exists(_native.LIB_PATH):
        __graft_entry__.build()
    lib = _native.lib()
    assert lib.exaspim_components_workspace_bytes(_native.int3((4, 5, 6))) >= 5 * 120
    assert lib.exaspim_components_workspace_bytes(_native.int3((0, 5, 6))) == 0
    assert lib.exaspim_components_workspace_bytes(_native.int3((2048, 1024, 1024))) == 0   # 2^31 voxels
    assert lib.exaspim_components_workspace_bytes(_native.int3((2047, 1024, 1024))) > 0
    fake = 0x10000
    dims = _native.int3((4, 5, 6))
    call = lib.exaspim_components
    assert call(fake, 0, 3, dims, 0.5, 0, fake, fake, fake, 0, None) == -3
    assert "workspace" in _native.last_error()
    assert call(fake, 0, 3, _native.int3((2048, 1024, 1024)), 0.5, 0, fake, fake, fake, 0, None) == -1
    assert call(fake, 0, 3, _native.int3((4, 0, 6)), 0.5, 0, fake, fake, fake, 0, None) == -1
    assert call(fake, 7, 3, dims, 0.5, 0, fake, fake, fake, 0, None) == -1
    assert call(fake, 0, 2, dims, 0.5, 0, fake, fake, fake, 0, None) == -1
    assert call(None, 0, 3, dims, 0.5, 0, fake, fake, fake, 0, None) == -1
    assert call(fake, 0, 3, dims, 0.5, 0, None, fake, fake, 0, None) == -1
    assert call(fake, 0, 3, dims, 0.5, 0, fake, None, fake, 0, None) == -1
    assert call(fake, 0, 3, dims, 0.5, 0, fake, fake, None, 0, None) == -1
    assert call(fake, 0, 3, dims, 0.5, 0, fake, fake, fake + 8, 0, None) == -1   # workspace not 16-byte aligned
    assert "misaligned" in _native.last_error()
