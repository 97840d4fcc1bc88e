"""
exaspim_label_pieces on the GPU (-m gpu) against tests/pieces_ref.py: the flood fill (A), or the per-label scipy
labelling (B) where the volume is large. Every C-ABI run writes into 0xFF-filled buffers between guard words and
every comparison is array_equal. Covered: the 13 neighbour directions across a tile corner, with one label and with
two; checkerboards; pieces separated by a plane of background or of another label; a diagonal snake through
several tiles; labels above K and negative, K = 0, an empty volume; 1 x 1 x 1, single-voxel axes, widths around
the tile's; a labels pointer that is only 4-byte aligned; dust at t - 1, t and t + 1 and the dust count; a volume
whose tile count exceeds one capped launch; determinism; every refusal (decided on the host, nothing launched);
the Python wrapper's four outputs; and the two consequences of DESIGN 6q on the device.
"""

import numpy as np
import pytest
import torch

import border_ref
import pieces_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference
from test_gpu_dbf import dev, guarded, intact  # noqa: F401  (fixture and helpers)

pytestmark = pytest.mark.gpu

CRAFTED = pieces_ref.crafted()


def run_pieces(dev, labels, k, dust=0, offset=0):      # noqa: F811
    """exaspim_label_pieces through the C ABI into guarded, poisoned buffers: (pieces, kept, dust pieces).
    offset: the labels start that many elements into their allocation (a pointer that is only 4-byte aligned)."""
    lib = _native.lib()
    shape = labels.shape
    n = int(np.prod(shape))
    dims = _native.int3(shape)
    held = torch.zeros(n + offset, dtype=torch.int32, device=dev)
    held[offset:] = torch.from_numpy(np.ascontiguousarray(labels).reshape(-1)).to(dev)
    t = held[offset:]
    need = lib.exaspim_label_pieces_workspace_bytes(dims)
    assert need >= 4 * n, _native.last_error()
    full, out = guarded(dev, n, torch.int32)
    st_full, state = guarded(dev, 2, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    rc = lib.exaspim_label_pieces(t.data_ptr(), dims, k, dust, out.data_ptr(), state.data_ptr(), ws.data_ptr(), need,
                                  None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(full, n, torch.int32) and intact(st_full, 2, torch.int32) and intact(ws_full, need, torch.uint8)
    np.testing.assert_array_equal(t.cpu().numpy().reshape(shape), labels)      # the input is only read
    kept, dusty = (int(v) for v in state.cpu())
    return out.cpu().numpy().reshape(shape), kept, dusty


def held_to(dev, labels, k, dust=0, oracle=pieces_ref.flood_fill, offset=0):      # noqa: F811
    want = oracle(labels, k, dust)
    got, kept, dusty = run_pieces(dev, labels, k, dust, offset)
    np.testing.assert_array_equal(got, want[0])
    assert kept == len(want[1]) and dusty == want[4]
    return want


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_the_crafted_cases(dev, name):      # noqa: F811
    labels, k, dust, kept = CRAFTED[name]
    want = held_to(dev, labels, k, dust)
    if kept is not None:
        assert len(want[1]) == kept


def test_checkerboards(dev):      # noqa: F811
    shape = (11, 17, 67)
    parity = (np.indices(shape).sum(axis=0) % 2 + 1).astype(np.int32)
    got, kept, dusty = run_pieces(dev, parity, 2)
    assert (kept, dusty) == (2, 0)
    np.testing.assert_array_equal(got, parity)      # voxel 0 is even: label 1 is piece 1
    even = np.zeros(shape, dtype=np.int32)
    even[::2, ::2, ::2] = 1
    got, kept, dusty = run_pieces(dev, even, 1)
    assert kept == 6 * 9 * 34 and dusty == 0
    np.testing.assert_array_equal(got[::2, ::2, ::2].reshape(-1), np.arange(1, kept + 1))
    assert int(got.sum()) == kept * (kept + 1) // 2
    got, kept, dusty = run_pieces(dev, even, 1, dust=2)
    assert (kept, dusty) == (0, 6 * 9 * 34) and not got.any()


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 70), (1, 19, 1), (21, 1, 1), (1, 9, 33), (9, 1, 65), (3, 5, 31),
                                   (3, 5, 32), (9, 9, 33), (2, 10, 63), (10, 3, 64), (9, 17, 65)])
def test_shapes(dev, shape):      # noqa: F811
    for seed in (4, 5):
        labels = pieces_ref.random_volume(seed, shape, fill=0.5)
        held_to(dev, labels, 3)
        held_to(dev, labels, 2, dust=3)


def test_a_labels_pointer_that_is_only_4_byte_aligned(dev):      # noqa: F811
    labels = pieces_ref.random_volume(7, (9, 10, 36), fill=0.5)
    for offset in (1, 3):
        held_to(dev, labels, 3, offset=offset)


def test_the_label_range(dev):      # noqa: F811
    labels = pieces_ref.random_volume(9, (9, 12, 40), k=4, fill=0.6)      # values -1 .. 5
    assert labels.min() == -1 and labels.max() == 5
    for k in (5, 4, 2, 1, 0, 2**31 - 1):
        want = held_to(dev, labels, k)
        assert (want[0] > 0).sum() == ((labels >= 1) & (labels <= k)).sum()
    got, kept, dusty = run_pieces(dev, np.zeros((9, 9, 40), dtype=np.int32), 3)
    assert (kept, dusty) == (0, 0) and not got.any()
    low = np.full((3, 9, 40), -2**31, dtype=np.int32)
    low[1] = 2**31 - 1
    got, kept, dusty = run_pieces(dev, low, 2**31 - 1)
    assert (kept, dusty) == (1, 0) and (got[1] == 1).all() and not got[0].any() and not got[2].any()


def test_dust(dev):      # noqa: F811
    for t in (2, 7, 30):
        labels = pieces_ref.dust_volume(t)
        for threshold, kept in ((0, 3), (1, 3), (t - 1, 3), (t, 2), (t + 1, 1), (t + 2, 0), (2**40, 0)):
            want = held_to(dev, labels, 1, threshold)
            assert len(want[1]) == kept and want[4] == 3 - kept
    labels = pieces_ref.random_volume(12, (10, 20, 70), fill=0.3)      # an even seed: voxel noise, much dust
    for threshold in (2, 3, 5, 9):
        want = held_to(dev, labels, 3, threshold)
        assert want[4] >= 1


def test_a_tile_count_beyond_one_capped_launch(dev):      # noqa: F811
    """(262152, 9, 9): 32769 x 2 tiles, more than the 65536 workgroups of one launch, against oracle (B). Seeded
    blocks in the first and last planes and around the plane where the second round of the launch begins."""
    shape = (262152, 9, 9)
    labels = np.zeros(shape, dtype=np.int32)
    for seed, z0 in enumerate((0, 262136, 262152 - 16, 131070)):
        labels[z0:z0 + 16] = pieces_ref.random_volume(20 + seed, (16, 9, 9), fill=0.5)
    labels[1000:250000, 4, 4] = 2      # one long piece through both rounds
    want = held_to(dev, labels, 3, oracle=pieces_ref.by_label)
    assert len(want[1]) > 20 and want[2].max() >= 249000
    held_to(dev, labels, 3, dust=4, oracle=pieces_ref.by_label)


def test_two_runs_give_the_same_bits(dev):      # noqa: F811
    labels = pieces_ref.random_volume(13, (20, 30, 70), fill=0.45)
    a, b = run_pieces(dev, labels, 3, 3), run_pieces(dev, labels, 3, 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    np.testing.assert_array_equal(a[0], pieces_ref.by_label(labels, 3, 3)[0])


def test_every_refusal_leaves_the_outputs_alone(dev):      # noqa: F811
    lib = _native.lib()
    shape = (3, 4, 5)
    dims = _native.int3(shape)
    labels = torch.ones(60 + 4, dtype=torch.int32, device=dev)
    need = lib.exaspim_label_pieces_workspace_bytes(dims)
    full, out = guarded(dev, 60, torch.int32)
    st_full, state = guarded(dev, 2, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)
    good = [labels.data_ptr(), dims, 1, 0, out.data_ptr(), state.data_ptr(), ws.data_ptr(), need, None]
    changes = [(0, None), (4, None), (5, None), (6, None), (1, _native.int3((3, 0, 5))),
               (1, _native.int3((2048, 1024, 1024))), (2, -1), (3, -1), (0, labels.data_ptr() + 2),
               (4, out.data_ptr() + 1), (5, state.data_ptr() + 2), (6, ws.data_ptr() + 8), (4, labels.data_ptr())]
    for at, value in changes:
        args = list(good)
        args[at] = value
        assert lib.exaspim_label_pieces(*args) == -1, (at, value)
        assert _native.last_error().startswith("label_pieces:"), _native.last_error()
    args = list(good)
    args[7] = need - 1
    assert lib.exaspim_label_pieces(*args) == -3 and "workspace" in _native.last_error()
    torch.cuda.synchronize()
    for buffer in (full, st_full, ws_full):
        assert bool((buffer == 0xFF).all())
    assert bool((labels == 1).all())
    assert lib.exaspim_label_pieces(*good) == 0      # and the good call is one
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [1, 0] and bool((out == 1).all())


def test_the_python_wrapper(dev):      # noqa: F811
    labels = pieces_ref.random_volume(15, (12, 20, 40), k=4, fill=0.5)      # values -1 .. 5: the default K is 5
    assert labels.max() == 5
    for k, dust in ((None, 0), (4, 0), (3, 4), (0, 0)):
        want = pieces_ref.flood_fill(labels, 5 if k is None else k, dust)
        got = inference.label_pieces(labels, n_labels=k, dust_threshold=dust)
        assert len(got) == 4 and all(isinstance(a, np.ndarray) for a in got)
        for a, b in zip(got, want[:4]):
            assert a.dtype == b.dtype and a.shape == b.shape
            np.testing.assert_array_equal(a, b)
    on_device = inference.label_pieces(torch.from_numpy(labels).to(dev), dust_threshold=2, return_device_tensors=True)
    want = pieces_ref.flood_fill(labels, 5, 2)
    for a, b in zip(on_device, want[:4]):
        assert isinstance(a, torch.Tensor) and a.device.type == "cuda"
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    want = pieces_ref.flood_fill(labels, 4, 2)
    pieces, state = inference._label_pieces_on_device(torch.from_numpy(labels).to(dev), 4, 2)
    np.testing.assert_array_equal(pieces.cpu().numpy(), want[0])
    assert state.cpu().tolist() == [len(want[1]), want[4]]
    empty = inference.label_pieces(np.zeros((2, 3, 4), dtype=np.int32))
    assert not empty[0].any() and [a.shape for a in empty[1:]] == [(0,)] * 3
    assert [a.dtype for a in empty] == [np.int32, np.int32, np.int64, np.int32]


def test_the_two_consequences_on_the_device(dev):      # noqa: F811
    labels = pieces_ref.random_volume(17, (10, 21, 45), fill=0.7)      # odd seed: blocks, deep pieces
    labels = np.where((labels >= 1) & (labels <= 3), labels, 0).astype(np.int32)
    for dust in (0, 20):
        pieces, piece_label, _, _ = inference.label_pieces(labels, n_labels=3, dust_threshold=dust)
        assert len(piece_label) >= 3 and (pieces > 0).any()
        for border in (False, True):      # (a)
            of_labels = inference.distance_to_boundary(labels, black_border=border)
            of_pieces = inference.distance_to_boundary(pieces, black_border=border)
            np.testing.assert_array_equal(of_pieces[pieces > 0], of_labels[pieces > 0])
        got = np.stack(inference.border_targets(pieces, n_labels=len(piece_label)), axis=1)      # (b)
        rows = np.stack(inference.border_targets(labels, n_labels=3), axis=1).astype(np.int64)
        number = pieces.reshape(-1)[rows[:, 1]]
        want = np.stack([number[number > 0], rows[number > 0, 1]], axis=1)
        want = want[np.lexsort((want[:, 1], want[:, 0]))]
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, border_ref.by_component(pieces, len(piece_label)))
        assert len(got) >= 3
        if dust:
            assert (number == 0).any()      # a target of the labels lay in dust
