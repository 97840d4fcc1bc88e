"""
The slab-by-slab watershed fragments on the GPU (-m gpu): exaspim_watershed_stream_slab, then
exaspim_components_stream_finish and _apply on the base descriptor, through the C ABI into guarded
buffers, against the whole-volume CPU oracle (tests/watershed_ref.py), labels and K array for array, under the cut
lists of test_watershed_stream_cpu.py; then WatershedStream and watershed_fragments_streaming against
watershed_fragments of the same tensor.
"""

import ctypes

import numpy as np
import pytest
import torch

import watershed_ref
from aind_exaspim_neuron_segmentation_amd import _native
from test_watershed_stream_cpu import BIG, KINDS, SHAPES, THRESHOLDS, affinities, cut_lists, whole

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements behind every buffer
POISON = -1234567
_DTYPES = {np.dtype(np.float32): torch.float32, np.dtype(np.float16): torch.float16}
_CODES = {torch.float32: _native.AFF_F32, torch.float16: _native.AFF_F16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def bounds_of(cuts, depth):
    return list(zip([0] + list(cuts), list(cuts) + [depth]))


class Guarded:
    """A device buffer of n elements with GUARD more behind it, all filled with the bytes of "fill"."""

    def __init__(self, dev, n, dtype, fill=0xA5):
        size = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((n + GUARD) * size,), fill, dtype=torch.uint8, device=dev)
        self.all = self.raw.view(dtype)
        self.n, self.fill = n, fill
        self.t = self.all[:n]

    def ptr(self):
        return self.all.data_ptr()

    def intact(self):
        return bool((self.raw[self.n * self.all.element_size():] == self.fill).all())


class AbiStream:
    """The caller's side of exaspim_watershed_stream: the descriptor and every buffer it points to, guarded and
    pre-filled with "fill" bytes (0xFF: NaN bits in the float plane, -1 in the ids)."""

    def __init__(self, dev, shape, low, high, min_size, capacity=None, fill=0xFF):
        self.dev, self.shape, self.fill = dev, tuple(shape), fill
        plane = shape[1] * shape[2]
        self.capacity = capacity = int(np.prod(shape)) if capacity is None else capacity
        self.id_parent = Guarded(dev, capacity + 1, torch.int32, fill)
        self.id_count = Guarded(dev, capacity + 1, torch.int64, fill)
        self.table = Guarded(dev, capacity + 1, torch.int32, fill)
        self.state = Guarded(dev, 4, torch.int32, fill)
        self.seam_ids = Guarded(dev, plane, torch.int32, fill)
        self.seam_bits = Guarded(dev, plane, torch.uint8, fill)
        self.seam_aff = Guarded(dev, plane, torch.float32, fill)
        self.buffers = [self.id_parent, self.id_count, self.table, self.state, self.seam_ids, self.seam_bits,
                        self.seam_aff]
        d = self.desc = _native.WatershedStreamDesc()
        b = d.base
        b.dims[:] = shape
        b.channels, b.threshold, b.capacity, b.min_size, b.next_z = 3, float("nan"), capacity, int(min_size), 0
        b.id_parent_dev, b.id_count_dev, b.table_dev = self.id_parent.ptr(), self.id_count.ptr(), self.table.ptr()
        b.state_dev, b.seam_ids_dev, b.seam_bits_dev = self.state.ptr(), self.seam_ids.ptr(), self.seam_bits.ptr()
        d.low, d.high, d.seam_aff_dev = float(np.float32(low)), float(np.float32(high)), self.seam_aff.ptr()

    def slab(self, part, z0, need=None, labels=None, workspace=None, dtype_code=None):
        """One exaspim_watershed_stream_slab on the contiguous (3, d, H, W) device tensor "part": (rc, labels)."""
        lib = _native.lib()
        dims = tuple(int(v) for v in part.shape[1:])
        if need is None:
            need = lib.exaspim_watershed_stream_slab_workspace_bytes(_native.int3(dims))
        lab = Guarded(self.dev, int(np.prod(dims)), torch.int32, 0x5A) if labels is None else labels
        ws = Guarded(self.dev, need, torch.uint8, self.fill) if workspace is None else workspace
        code = _CODES[part.dtype] if dtype_code is None else dtype_code
        rc = lib.exaspim_watershed_stream_slab(ctypes.byref(self.desc), part.data_ptr(), code, _native.int3(dims), z0,
                                               lab.ptr(), ws.ptr(), need, None)
        self.buffers += [lab, ws]
        return rc, lab

    def finish(self):
        lib = _native.lib()
        need = lib.exaspim_components_stream_finish_workspace_bytes(self.capacity)
        ws = Guarded(self.dev, need, torch.uint8, self.fill)
        self.buffers.append(ws)
        rc = lib.exaspim_components_stream_finish(ctypes.byref(self.desc.base), ws.ptr(), need, None)
        assert rc == 0, _native.last_error()
        used, overflow, k, _ = (int(v) for v in self.state.t.cpu())
        return used, overflow, k

    def apply(self, lab):
        rc = _native.lib().exaspim_components_stream_apply(ctypes.byref(self.desc.base), lab.ptr(), lab.n, None)
        assert rc == 0, _native.last_error()

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(b.intact() for b in self.buffers)


def on_device(dev, aff, offset=0):
    """aff as a contiguous device tensor whose base pointer is "offset" elements past a 16-byte boundary; the
    tensor it is a view of comes along so that it can be compared with its input afterwards."""
    aff = np.array(aff, order="C")      # a copy: the shared inputs are read-only
    flat = torch.zeros(aff.size + offset, dtype=_DTYPES[aff.dtype], device=dev)
    flat[offset:] = torch.from_numpy(aff).to(dev).reshape(-1)
    return flat[offset:].view(aff.shape), flat


def stream(dev, aff, low, high, min_size, cuts, offset=0, fill=0xFF, capacity=None):
    """(labels, K, provisional, ids used) of the slabs that "cuts" make of aff, through the C ABI."""
    aff = np.asarray(aff)
    shape = aff.shape[1:]
    s = AbiStream(dev, shape, low, high, min_size, capacity, fill)
    parts = []
    for z0, z1 in bounds_of(cuts, shape[0]):
        part, keep = on_device(dev, aff[:, z0:z1], offset)
        before = keep.clone()
        rc, lab = s.slab(part, z0)
        assert rc == 0, _native.last_error()
        assert s.desc.base.next_z == z1
        parts.append((lab, part, keep, before))
    used, overflow, k = s.finish()
    assert not overflow
    provisional = np.concatenate([lab.t.cpu().numpy() for lab, *_ in parts]).reshape(shape)
    for lab, *_ in parts:
        s.apply(lab)
    final = np.concatenate([lab.t.cpu().numpy() for lab, *_ in parts]).reshape(shape)
    assert s.guards_intact()
    assert all(torch.equal(keep.view(torch.uint8), before.view(torch.uint8)) for _, _, keep, before in parts)
    assert 0 <= provisional.min(initial=0) and provisional.max(initial=0) <= used
    table = s.table.t[: used + 1].cpu().numpy()
    np.testing.assert_array_equal(table[provisional], final)
    return final, k, provisional, used


def check(dev, aff, low, high, min_size, cuts, want=None, **kw):
    if want is None:
        want = watershed_ref.fragments(aff, low, high, min_size)
    got, k, _, _ = stream(dev, aff, low, high, min_size, cuts, **kw)
    assert got.dtype == np.int32 and k == want[1] == int(got.max(initial=0))
    np.testing.assert_array_equal(got, want[0])
    return got, k


# ---- 1. the CPU cases -------------------------------------------------------------------------------------
@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_random_affinities_under_every_cut_list(dev, kind, shape, low, high):
    """(5, 6, 7) and (9, 9, 33) take the scalar path (widths that are no multiple of the vector), and so does
    (17, 17, 65); with a depth of 9 or 17 the slab's last plane is a tile's halo plane."""
    for cuts in cut_lists(shape[0]).values():
        check(dev, affinities(kind, shape), low, high, 0, cuts, want=whole(kind, shape, low, high))


WIDE = (17, 16, 64)      # the 16-byte loads: a width of whole vectors of either type


def wide(kind, dtype=np.float32):
    a = np.ascontiguousarray(affinities(kind, BIG, dtype)[:, :, :16, :64])
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("kind", KINDS)
def test_the_wide_loads_and_a_base_pointer_off_by_one_element(dev, kind, dtype):
    aff = wide(kind, dtype)
    for low, high in THRESHOLDS:
        want = watershed_ref.fragments(aff, low, high, 0)
        for cuts in cut_lists(WIDE[0]).values():
            check(dev, aff, low, high, 0, cuts, want=want)
        check(dev, aff, low, high, 0, [8], want=want, offset=1)      # the scalar path on the same input
        check(dev, aff, low, high, 0, [9], want=want, offset=1)


@pytest.mark.parametrize("low,high", THRESHOLDS)
@pytest.mark.parametrize("kind", KINDS)
def test_float16_eighths_with_tied_maxima(dev, kind, low, high):
    for shape in SHAPES:
        for cuts in cut_lists(shape[0]).values():
            check(dev, affinities(kind, shape, np.float16), low, high, 0, cuts,
                  want=whole(kind, shape, low, high, dtype=np.float16))


@pytest.mark.parametrize("min_size", [1, 5, 40])
def test_the_size_filter_sees_whole_fragments(dev, min_size):
    for cuts in cut_lists(BIG[0]).values():
        check(dev, affinities("smooth", BIG), 0.3, 0.7, min_size, cuts, want=whole("smooth", BIG, 0.3, 0.7, min_size))


# ---- 2. hand-built lines along z across a seam ------------------------------------------------------------------
def every_cut(depth):
    return [[c] for c in range(1, depth)] + [list(range(1, depth))]


@pytest.mark.parametrize("name,values,low,high,min_size,labels", watershed_ref.LINES, ids=[c[0] for c in watershed_ref.LINES])
def test_lines_along_z_cut_everywhere(dev, name, values, low, high, min_size, labels):
    """Strict low and inclusive high, NaN and +-inf in the value that gets carried, ties (-z first, +z last), the
    size filter: each line with a seam at every position, so every value is carried once and handed on once."""
    aff = watershed_ref.line_affinities(0, values)
    for dtype in (np.float32, np.float16):
        a = aff.astype(dtype)
        want = watershed_ref.fragments(a, low, high, min_size)
        if dtype == np.float32:
            assert want[0].ravel().tolist() == labels
        for cuts in every_cut(len(values)):
            check(dev, a, low, high, min_size, cuts, want=want)


def test_a_voxel_whose_only_on_edge_crosses_the_seam(dev):
    """On each side: 0.5 at the seam is the one eligible edge of both its ends."""
    aff = np.zeros((3, 4, 3, 5), np.float32)
    aff[0, 1, 2, 4] = 0.5
    got, k = check(dev, aff, 0.1, 0.9999, 0, [2])
    assert k == 1 and got[1, 2, 4] == got[2, 2, 4] == 1 and np.count_nonzero(got) == 2
    _, k = check(dev, aff, 0.1, 0.9999, 2, [2])
    assert k == 0
    # below the seam the edge is the lower end's steepest; above, only the upper end's choice switches it on
    aff[0, 0, 2, 4] = 0.8
    got, k = check(dev, aff, 0.1, 0.9999, 0, [2])
    assert k == 1 and got[0, 2, 4] == got[1, 2, 4] == got[2, 2, 4] == 1
    _, _, provisional, used = stream(dev, aff, 0.1, 0.9999, 0, [2])
    assert used == 2 and np.count_nonzero(provisional) == 3


def test_the_volumes_last_plane_with_poisoned_z_entries(dev):
    aff = np.array(affinities("uniform", (9, 9, 33)))
    want = whole("uniform", (9, 9, 33), 0.3, 0.7)
    for poison in (np.nan, np.inf, 1.0, -np.inf):
        aff[0, -1] = poison
        for cuts in ([], [8], [4]):
            check(dev, aff, 0.3, 0.7, 0, cuts, want=want)


def test_high_at_or_below_low(dev):
    aff = affinities("uniform", (9, 9, 33))
    for low, high in ((0.5, 0.5), (0.5, 0.2), (-1.0, -2.0)):
        check(dev, aff, low, high, 0, [8])
        check(dev, aff, low, high, 0, [3, 4])


@pytest.mark.parametrize("shape", [(9, 1, 1), (1, 33, 65), (5, 1, 9), (6, 7, 1), (1, 1, 1)])
def test_a_dimension_of_one(dev, shape):
    aff = np.random.default_rng(7).random((3,) + shape).astype(np.float32)
    check(dev, aff, 0.3, 0.7, 0, list(range(1, shape[0])))
    check(dev, aff, 0.3, 0.7, 0, [])
    check(dev, np.ones((3,) + shape, np.float32), 0.1, 0.9999, 0, list(range(1, shape[0])))


@pytest.mark.parametrize("shape,cut", [((262152, 9, 9), 262147), ((262160, 9, 4), 262149)], ids=["scalar", "vector"])
def test_a_slab_with_more_tiles_than_one_capped_launch_takes(dev, shape, cut):
    """The shapes of test_gpu_watershed.py's test_grid_stride_over_tiles, cut so that the first slab alone has
    65538 tiles, more than the 65536 workgroups a launch is capped at: the mask kernel strides, and tiles of its
    second trip hold the slab's last plane and hand on the seam."""
    assert -(-cut // 8) * -(-shape[1] // 8) * -(-shape[2] // 32) > 65536 and cut % 8 != 0
    aff = np.random.default_rng(23).random((3,) + shape, dtype=np.float32)
    want = watershed_ref.fragments(aff, 0.3, 0.7, 0)
    assert ((want[0][cut - 1] == want[0][cut]) & (want[0][cut] > 0)).any()
    check(dev, aff, 0.3, 0.7, 0, [cut], want=want)


# ---- 3. robustness and behaviour ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x7F, 0x00, 0xA5])
def test_nothing_is_read_before_it_is_written(dev, fill):
    """Workspace, id tables and all three carried planes pre-filled: 0xFF is NaN bits in the float plane, all bits
    set in the seam bits and -1 in the ids; 0x7F bytes are a NaN as well."""
    for cuts in ([8], [9], list(range(1, 17))):
        check(dev, affinities("uniform", BIG), 0.3, 0.7, 0, cuts, want=whole("uniform", BIG, 0.3, 0.7), fill=fill)
        check(dev, wide("uniform"), 0.3, 0.7, 0, cuts, fill=fill)


def test_purity_across_cut_lists_and_runs(dev):
    aff = wide("saturated")
    a = stream(dev, aff, 0.1, 0.9999, 3, [8])
    b = stream(dev, aff, 0.1, 0.9999, 3, [1, 4, 5, 11, 16])
    c = stream(dev, aff, 0.1, 0.9999, 3, [8])
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1] == b[1] == c[1]
    assert a[2].tobytes() == c[2].tobytes() and a[3] == c[3]


def test_z0_zero_starts_a_new_volume_on_used_state(dev):
    aff = affinities("uniform", (9, 9, 33))
    s = AbiStream(dev, (9, 9, 33), 0.3, 0.7, 0)
    for _ in range(2):      # the second volume runs on the first one's state, next_z put back by the caller
        s.desc.base.next_z = 0
        labs = []
        for z0, z1 in bounds_of([4], 9):
            rc, lab = s.slab(on_device(dev, aff[:, z0:z1])[0], z0)
            assert rc == 0, _native.last_error()
            labs.append(lab)
        _, overflow, k = s.finish()
        for lab in labs:
            s.apply(lab)
        got = np.concatenate([lab.t.cpu().numpy() for lab in labs]).reshape(9, 9, 33)
        want = whole("uniform", (9, 9, 33), 0.3, 0.7)
        assert not overflow and k == want[1]
        np.testing.assert_array_equal(got, want[0])
    assert s.guards_intact()


def test_capacity_overflow_is_flagged_and_named(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = affinities("uniform", BIG)
    s = AbiStream(dev, BIG, 0.3, 0.7, 0, capacity=4)
    for z0, z1 in bounds_of([8], BIG[0]):
        rc, lab = s.slab(on_device(dev, aff[:, z0:z1])[0], z0)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(lab.t.min()) >= 0 and int(lab.t.max()) <= 4
    used, overflow, _ = s.finish()
    assert (used, overflow) == (4, 1) and s.guards_intact()
    ws = inference.WatershedStream(BIG, 0.3, 0.7, device=dev, id_capacity=4)
    t = torch.from_numpy(np.array(aff)).to(dev)
    ws.push(t[:, :8])
    ws.push(t[:, 8:])
    with pytest.raises(RuntimeError, match="WatershedStream.*id_capacity=4"):
        ws.finish()
    check(dev, aff, 0.3, 0.7, 0, [8], want=whole("uniform", BIG, 0.3, 0.7))      # the device is fine


def test_every_refusal_comes_before_any_launch_and_leaves_the_descriptor(dev):
    lib = _native.lib()
    shape = (9, 9, 33)
    aff = affinities("uniform", shape)
    s = AbiStream(dev, shape, 0.3, 0.7, 0)
    first, _ = on_device(dev, aff[:, :4])
    second, _ = on_device(dev, aff[:, 4:])
    lab = Guarded(dev, 5 * 9 * 33, torch.int32, 0x5A)
    need = lib.exaspim_watershed_stream_slab_workspace_bytes(_native.int3((5, 9, 33)))
    assert need == lib.exaspim_components_stream_slab_workspace_bytes(_native.int3((5, 9, 33)))
    ws = Guarded(dev, need, torch.uint8, 0xA5)
    assert lib.exaspim_watershed_stream_slab_workspace_bytes(_native.int3((0, 9, 33))) == 0

    def snapshot():
        return bytes(s.desc)

    def refused(rc, message, code=-1):
        assert rc == code and message in _native.last_error(), (rc, _native.last_error())
        torch.cuda.synchronize()
        assert snapshot() == before and bool((lab.raw == 0x5A).all()) and bool((ws.raw == 0xA5).all())

    before = snapshot()
    refused(s.slab(second, 4, labels=lab, workspace=ws, need=need)[0], "z order")      # the first slab starts at 0
    assert s.slab(first, 0)[0] == 0
    torch.cuda.synchronize()
    state = s.state.t.cpu().tolist()
    before = snapshot()
    args = dict(labels=lab, workspace=ws, need=need)
    refused(s.slab(second, 0, **args)[0], "z order")
    refused(s.slab(second, 5, **args)[0], "z order")
    refused(s.slab(on_device(dev, aff[:, 3:])[0], 4, **args)[0], "leave the volume")
    refused(s.slab(on_device(dev, aff[:, 4:, :, :32])[0], 4, **args)[0], "(y, x)")
    refused(s.slab(on_device(dev, aff[:, 4:, :8])[0], 4, **args)[0], "(y, x)")
    refused(s.slab(second, 4, dtype_code=7, **args)[0], "aff_dtype")
    refused(s.slab(second, 4, labels=lab, workspace=ws, need=need - 1)[0], "workspace", code=-3)
    rc = lib.exaspim_watershed_stream_slab(ctypes.byref(s.desc), second.data_ptr(), _native.AFF_F32,
                                           _native.int3((5, 9, 33)), 4, lab.ptr() + 2, ws.ptr(), need, None)
    refused(rc, "misaligned")
    rc = lib.exaspim_watershed_stream_slab(ctypes.byref(s.desc), second.data_ptr(), _native.AFF_F32,
                                           _native.int3((5, 9, 33)), 4, lab.ptr(), ws.ptr() + 4, need, None)
    refused(rc, "misaligned")
    rc = lib.exaspim_watershed_stream_slab(ctypes.byref(s.desc), None, _native.AFF_F32, _native.int3((5, 9, 33)), 4,
                                           lab.ptr(), ws.ptr(), need, None)
    refused(rc, "NULL")
    rc = lib.exaspim_watershed_stream_slab(None, second.data_ptr(), _native.AFF_F32, _native.int3((5, 9, 33)), 4,
                                           lab.ptr(), ws.ptr(), need, None)
    refused(rc, "NULL stream descriptor")

    def with_field(setter, message):
        """One field of the descriptor made wrong for one call, put back, and the call refused."""
        nonlocal before
        good = snapshot()
        setter()
        before = snapshot()
        refused(s.slab(second, 4, **args)[0], message)
        ctypes.memmove(ctypes.addressof(s.desc), good, len(good))
        before = good

    def set_base(name, value):
        return lambda: setattr(s.desc.base, name, value)

    with_field(set_base("channels", 1), "channels must be 3")
    with_field(set_base("channels", 2), "channels must be 3")
    with_field(lambda: setattr(s.desc, "seam_aff_dev", None), "seam_aff_dev")
    with_field(lambda: setattr(s.desc, "seam_aff_dev", s.seam_aff.ptr() + 2), "seam_aff_dev")
    with_field(lambda: setattr(s.desc, "low", float("nan")), "NaN")
    with_field(lambda: setattr(s.desc, "high", float("nan")), "NaN")
    with_field(set_base("capacity", 0), "capacity")
    with_field(set_base("seam_bits_dev", None), "NULL device buffer")
    with_field(set_base("id_count_dev", s.id_count.ptr() + 4), "misaligned device buffer")
    with_field(set_base("next_z", 10), "next_z")
    assert s.state.t.cpu().tolist() == state

    # and the stream still goes on from where it was
    rc, rest = s.slab(second, 4)
    assert rc == 0
    _, overflow, k = s.finish()
    want = whole("uniform", shape, 0.3, 0.7)
    assert not overflow and k == want[1]
    s.apply(rest)
    np.testing.assert_array_equal(rest.t.cpu().numpy().reshape(5, 9, 33), want[0][4:])
    assert s.guards_intact()


# ---- 4. through Python -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_watershed_stream_equals_watershed_fragments_of_the_same_tensor(dev, dtype):
    from aind_exaspim_neuron_segmentation_amd import inference

    for aff in (wide("smooth", dtype), affinities("saturated", BIG, dtype)):
        t = torch.from_numpy(np.array(aff)).to(dev)
        for min_size in (0, 5):
            want = inference.watershed_fragments(t, 0.3, 0.7, min_size, return_device_tensor=True)
            for cuts in ([8], [9], [1, 4, 5, 11, 16]):
                ws = inference.WatershedStream(aff.shape[1:], 0.3, 0.7, min_size, device=dev)
                parts = [ws.push(t[:, z0:z1]) for z0, z1 in bounds_of(cuts, aff.shape[1])]
                assert ws.next_z == aff.shape[1]
                table, k = ws.finish()
                got = torch.cat([ws.apply(p) for p in parts])
                assert torch.equal(got, want) and k == int(want.max()) and ws.ids_used >= k
                assert table.shape == (ws.id_capacity + 1,)


def test_watershed_fragments_streaming_from_a_host_array(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    aff = affinities("smooth", BIG)
    want = inference.watershed_fragments(np.array(aff), 0.3, 0.7, 3)
    np.testing.assert_array_equal(want, whole("smooth", BIG, 0.3, 0.7, 3)[0])
    for resident in (True, False):
        got = inference.watershed_fragments_streaming(aff, 0.3, 0.7, 3, slab_depth=7, keep_labels_resident=resident)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want)
    blocks = []
    table, k = inference.watershed_fragments_streaming(aff, 0.3, 0.7, 3, slab_depth=7,
                                                       write_block=lambda z0, z1, b: blocks.append((z0, z1, b.copy())))
    assert [(b[0], b[1]) for b in blocks] == [(z, min(z + 7, 17)) for z in range(0, 17, 7)]
    np.testing.assert_array_equal(table[np.concatenate([b[2] for b in blocks])], want)
    assert k == int(want.max())
    got = inference.watershed_fragments_streaming(aff.astype(np.float16), 0.3, 0.7, 3, slab_depth=1)
    np.testing.assert_array_equal(got, watershed_ref.fragments(aff.astype(np.float16), 0.3, 0.7, 3)[0])
