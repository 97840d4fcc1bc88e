"""
exaspim_border_targets and inference.border_targets on the GPU (-m gpu), compared as sorted sets with the brute
force of tests/border_ref.py (tests/test_border_ref_cpu.py holds it to the per-component distance transform):
the shapes around the wave (64), the workgroup (256 face pixels) and a plane width of 63 / 64 / 65, a volume with
more face pixels than one launch of 2048 workgroups covers, the crafted planes, a capacity smaller than the
count, every refusal, determinism, the Python wrapper's sorted and deduplicated output, and the seam property.
Every run through the C ABI writes into buffers pre-filled with 0xFF bytes whose guard words must not change.
Nothing here provokes a fault: every refused call is rejected on the host before a launch.
"""

import numpy as np
import pytest
import torch

import border_ref
from aind_exaspim_neuron_segmentation_amd import _native, inference
from test_gpu_dbf import dev, guarded, intact  # noqa: F401  (fixture and helpers)

pytestmark = pytest.mark.gpu

GRID, THREADS = 2048, 256      # border.hip: the launches are capped at GRID workgroups of THREADS pixels and stride
E_INVALID, E_WORKSPACE = -1, -3


def face_pixels(shape):
    d, h, w = shape
    return 2 * (h * w + d * w + d * h)


def run(dev, labels, k, capacity=None):      # noqa: F811
    """exaspim_border_targets into guarded 0xFF buffers: (rows written as an (n, 2) array, the count)."""
    lib = _native.lib()
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    shape = labels.shape
    dims = _native.int3(shape)
    capacity = face_pixels(shape) if capacity is None else capacity
    t = torch.from_numpy(labels).to(dev)
    need = lib.exaspim_border_targets_workspace_bytes(dims)
    assert need >= 24 * face_pixels(shape), _native.last_error()
    full_l, out_l = guarded(dev, capacity, torch.int32)
    full_v, out_v = guarded(dev, capacity, torch.int32)
    full_s, state = guarded(dev, 2, torch.int32)
    full_w, ws = guarded(dev, need, torch.uint8)
    rc = lib.exaspim_border_targets(t.data_ptr(), dims, k, out_l.data_ptr(), out_v.data_ptr(), capacity,
                                    state.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(full_l, capacity, torch.int32) and intact(full_v, capacity, torch.int32)
    assert intact(full_s, 2, torch.int32) and intact(full_w, need, torch.uint8)
    np.testing.assert_array_equal(t.cpu().numpy(), labels)      # the input is only read
    count, spare = (int(v) for v in state.cpu())
    assert spare == 0 and count >= 0
    rows = np.stack([out_l.cpu().numpy(), out_v.cpu().numpy()], axis=1).astype(np.int64)
    assert (rows[min(count, capacity):] == -1).all()      # nothing written past the count or the capacity
    return rows[:min(count, capacity)], count


def as_sorted(rows):
    return np.array(sorted(map(tuple, rows.tolist())), dtype=np.int64).reshape(-1, 2)


def check(dev, labels, k, oracle=border_ref.brute_force):      # noqa: F811
    rows, count = run(dev, labels, k)
    want = oracle(labels, k)
    assert count == len(rows)
    np.testing.assert_array_equal(as_sorted(rows), want)      # as a sorted list: no row twice either
    return want


@pytest.mark.parametrize("shape", border_ref.SHAPES, ids=str)
@pytest.mark.parametrize("seed", [0, 1])
def test_seeded_volumes_around_the_wave_and_the_workgroup(dev, shape, seed):      # noqa: F811
    assert {face_pixels(s) for s in border_ref.SHAPES} >= {254, 256, 258}      # the workgroup at -2, 0, +2
    check(dev, border_ref.random_volume(100 + 2 * border_ref.SHAPES.index(shape) + seed, shape), 5)


def test_more_face_pixels_than_one_capped_launch(dev):      # noqa: F811
    """
    (1, 520, 520) has 542 880 face pixels, more than the 2048 x 256 = 524 288 one trip covers: the second z face's
    last rows and all four side faces lie in the second trip of every launch. The brute force is quadratic, so
    the oracle here is the per-component distance transform, which test_border_ref_cpu.py holds to it.
    """
    shape = (1, 520, 520)
    assert GRID * THREADS < face_pixels(shape) < 2 * GRID * THREADS
    labels = border_ref.random_volume(11, shape)      # blocks of 3: a few thousand components per face
    want = check(dev, labels, 5, oracle=border_ref.by_component)
    assert len(want) > 1000
    solid = np.full(shape, 2, dtype=np.int32)      # one component per face, e up to 260^2, unions across both trips
    rows, count = run(dev, solid, 2)
    # z0 and z1 coincide: the centre; the four side faces are lines of e = 1, and x0's first voxel is y0's
    assert count == 4 and as_sorted(rows).tolist() == [[2, 0], [2, 519], [2, 259 * 520 + 259], [2, 519 * 520]]
    np.testing.assert_array_equal(as_sorted(rows), border_ref.by_component(solid, 2))


@pytest.mark.parametrize("name", sorted(border_ref.crafted()))
def test_crafted_planes(dev, name):      # noqa: F811
    labels, k, _ = border_ref.crafted()[name]
    want = check(dev, labels, k)
    if name == "an empty volume":
        assert len(want) == 0
    if name == "an edge and a corner":
        assert len(want) == 3      # one row each, not two or three


def test_a_capacity_smaller_than_the_count(dev):      # noqa: F811
    labels = border_ref.random_volume(5, (7, 9, 70))
    want = border_ref.brute_force(labels, 5)
    assert len(want) > 40
    for capacity in (0, 1, 17, len(want) - 1, len(want)):
        rows, count = run(dev, labels, 5, capacity=capacity)      # run() holds the guards and the unwritten rows
        assert count == len(want) and len(rows) == min(capacity, len(want))
        assert set(map(tuple, rows.tolist())) <= set(map(tuple, want.tolist()))
        assert len(set(map(tuple, rows.tolist()))) == len(rows)


def test_two_runs_give_the_same_set(dev):      # noqa: F811
    labels = border_ref.random_volume(9, (3, 66, 65))
    first, _ = run(dev, labels, 5)
    second, _ = run(dev, labels, 5)
    np.testing.assert_array_equal(as_sorted(first), as_sorted(second))


def test_refusals(dev):      # noqa: F811
    lib = _native.lib()
    shape = (3, 4, 5)
    dims = _native.int3(shape)
    labels = torch.ones(shape, dtype=torch.int32, device=dev)
    need = lib.exaspim_border_targets_workspace_bytes(dims)
    capacity = face_pixels(shape)
    full_l, out_l = guarded(dev, capacity, torch.int32)
    full_v, out_v = guarded(dev, capacity, torch.int32)
    full_s, state = guarded(dev, 2, torch.int32)
    full_w, ws = guarded(dev, need + 16, torch.uint8)
    good = dict(labels=labels.data_ptr(), dims=dims, k=1, out_l=out_l.data_ptr(), out_v=out_v.data_ptr(),
                capacity=capacity, state=state.data_ptr(), ws=ws.data_ptr(), bytes=need)

    def call(**changes):
        a = dict(good, **changes)
        return lib.exaspim_border_targets(a["labels"], a["dims"], a["k"], a["out_l"], a["out_v"], a["capacity"],
                                          a["state"], a["ws"], a["bytes"], None)

    invalid = [dict(labels=None), dict(out_l=None), dict(out_v=None), dict(state=None), dict(ws=None),
               dict(dims=_native.int3((0, 4, 5))), dict(dims=_native.int3((3, -1, 5))),
               dict(dims=_native.int3((2048, 2048, 512))), dict(k=-1), dict(capacity=-1),
               dict(labels=labels.data_ptr() + 2), dict(out_l=out_l.data_ptr() + 1), dict(out_v=out_v.data_ptr() + 2),
               dict(state=state.data_ptr() + 2), dict(ws=ws.data_ptr() + 8)]
    for changes in invalid:
        assert call(**changes) == E_INVALID, changes
        assert _native.last_error().startswith("border_targets:"), changes
    assert call(bytes=need - 1) == E_WORKSPACE and "workspace" in _native.last_error()
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((0, 1, 1))) == 0
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((2048, 2048, 512))) == 0
    # more than 2^31 - 1 face pixels in a volume of fewer voxels
    assert lib.exaspim_border_targets_workspace_bytes(_native.int3((1, 1, 2**30))) == 0
    assert "face pixels" in _native.last_error()
    torch.cuda.synchronize()
    for full, n, dtype in ((full_l, capacity, torch.int32), (full_v, capacity, torch.int32), (full_s, 2, torch.int32),
                           (full_w, need + 16, torch.uint8)):
        assert bool((full.view(torch.uint8) == 0xFF).all()), "a refused call touched an output"
    # the two arrays may be NULL where the capacity is 0
    assert call(out_l=None, out_v=None, capacity=0) == 0
    torch.cuda.synchronize()
    assert int(state.cpu()[0]) == len(border_ref.brute_force(np.ones(shape, dtype=np.int32), 1))


def test_through_python_sorted_and_deduplicated(dev):      # noqa: F811
    labels = border_ref.random_volume(21, (7, 9, 70))
    want = border_ref.brute_force(labels, 5)
    got = inference.border_targets(labels)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int32 and a.ndim == 1 for a in got)
    np.testing.assert_array_equal(np.stack(got, axis=1), want)
    on_device = inference.border_targets(torch.from_numpy(labels).to(dev), n_labels=3, return_device_tensors=True)
    assert all(t.device.type == "cuda" and t.dtype == torch.int32 for t in on_device)
    np.testing.assert_array_equal(torch.stack(on_device, dim=1).cpu().numpy(), border_ref.brute_force(labels, 3))
    corner, k, _ = border_ref.crafted()["an edge and a corner"]
    np.testing.assert_array_equal(np.stack(inference.border_targets(corner), axis=1), border_ref.brute_force(corner, k))
    empty = inference.border_targets(np.zeros((3, 4, 5), dtype=np.int32))
    assert all(a.shape == (0,) and a.dtype == np.int32 for a in empty)
    thin = border_ref.random_volume(23, (1, 5, 5))      # z0 and z1 coincide: every pair once
    np.testing.assert_array_equal(np.stack(inference.border_targets(thin), axis=1), border_ref.brute_force(thin, 5))


@pytest.mark.parametrize("s", [1, 33, 64, 68])
def test_the_two_sides_of_a_seam_pick_the_same_voxels(dev, s):      # noqa: F811
    """
    A = V[:, :, :s + 1] and B = V[:, :, s:] share the plane x = s. A voxel on the rim of that plane lies on
    another face as well and may be that face's target, so the comparison is over the plane's interior, where a
    target can only be the plane's own; the volume is made of blocks of 3, whose centres lie there.
    """
    volume = border_ref.random_volume(31, (6, 9, 70))
    d, h, w = volume.shape
    a, b = np.ascontiguousarray(volume[:, :, :s + 1]), np.ascontiguousarray(volume[:, :, s:])

    def inside(pairs, pw, x):
        out = set()
        for label, v in pairs:
            z, y, px = v // (h * pw), v // pw % h, v % pw
            if px == x and 0 < z < d - 1 and 0 < y < h - 1:
                out.add((int(label), int((z * h + y) * w + s)))
        return out

    left = inside(zip(*inference.border_targets(a, n_labels=5)), s + 1, s)
    right = inside(zip(*inference.border_targets(b, n_labels=5)), w - s, 0)
    assert left == right and len(left) >= 2
    assert left == inside(border_ref.face_targets(a, 5, 5), s + 1, s)
