"""
exaspim_geodesic_begin / _sweeps / _farthest and inference.geodesic_field on the GPU (-m gpu). Every field is
compared with array_equal on its int32 bit patterns against the vectorised relaxation of
tests/geodesic_ref.py (tests/test_geodesic_ref_cpu.py holds it to a float32 heap Dijkstra): lines along every
axis across the tile edges, diagonals through tile corners, a serpentine that re-enters tiles, touching
labels, an id in two pieces, labels outside 1..K, missing and invalid sources, degenerate volumes, seeded
volumes in both modes, the farthest table, a volume with more tiles than one capped launch, determinism,
every refusal, and the chain from agglomerate_affinities to the distance-from-root field on the device. Every
run through the C ABI writes into buffers pre-filled with 0xFF bytes between guard words that must not
change. Nothing here provokes a fault: every refused call is rejected on the host before a launch.
"""

import numpy as np
import pytest
import torch

import geodesic_ref as ref
import holes_ref
from aind_exaspim_neuron_segmentation_amd import _native

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)      # (z, y, x) of the LDS pass
GUARD = 64             # elements around every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def guarded(dev, n, dtype):
    """A 0xFF-filled buffer of GUARD + n + GUARD elements and the view of its n middle ones."""
    full = torch.full(((n + 2 * GUARD) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8,
                      device=dev)
    return full, full.view(dtype)[GUARD:GUARD + n]


def intact(full, n, dtype):
    """The guard elements on both sides of a guarded() buffer still hold 0xFF bytes."""
    typed = full.view(dtype)
    return bool((typed[:GUARD].view(torch.uint8) == 0xFF).all() and (typed[GUARD + n:].view(torch.uint8) == 0xFF).all())


def run_geodesic(dev, labels, sources, cost=None, sweeps_per_call=4, limit=4096):
    """
    begin, sweeps until state[0] == 0, farthest: through the C ABI into guarded, poisoned buffers.
    Returns (field, far_value, far_index, invalid rows, sweeps launched).
    """
    lib = _native.lib()
    labels = np.array(labels, dtype=np.int32)
    sources = np.array(sources, dtype=np.int32)
    shape, k = labels.shape, len(sources) - 1
    n = int(np.prod(shape))
    dims = _native.int3(shape)
    lab = torch.from_numpy(labels).to(dev)
    src = torch.from_numpy(sources).to(dev)
    cst = None if cost is None else torch.from_numpy(np.array(cost, dtype=np.float32)).to(dev)
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    assert need >= 32, _native.last_error()
    field_full, field = guarded(dev, n, torch.float32)
    state_full, state = guarded(dev, 2, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    rc = lib.exaspim_geodesic_begin(lab.data_ptr(), dims, src.data_ptr(), k, field.data_ptr(), state.data_ptr(),
                                    ws.data_ptr(), need, None)
    assert rc == 0, _native.last_error()
    flagged, invalid = state.cpu().tolist()
    launched = 0
    while flagged:
        assert launched < limit, "no convergence"
        rc = lib.exaspim_geodesic_sweeps(lab.data_ptr(), None if cst is None else cst.data_ptr(), dims, k,
                                         field.data_ptr(), sweeps_per_call, state.data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        launched += sweeps_per_call
        flagged, still_invalid = state.cpu().tolist()
        assert still_invalid == invalid
    far_need = lib.exaspim_geodesic_farthest_workspace_bytes(k)
    value_full, value = guarded(dev, k + 1, torch.float32)
    index_full, index = guarded(dev, k + 1, torch.int32)
    far_ws_full, far_ws = guarded(dev, far_need, torch.uint8)
    rc = lib.exaspim_geodesic_farthest(lab.data_ptr(), field.data_ptr(), dims, k, value.data_ptr(), index.data_ptr(),
                                       far_ws.data_ptr(), far_need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(field_full, n, torch.float32) and intact(state_full, 2, torch.int32)
    assert intact(ws_full, need, torch.uint8) and intact(far_ws_full, far_need, torch.uint8)
    assert intact(value_full, k + 1, torch.float32) and intact(index_full, k + 1, torch.int32)
    np.testing.assert_array_equal(lab.cpu().numpy(), labels)      # the inputs are only read
    np.testing.assert_array_equal(src.cpu().numpy(), sources)
    return field.cpu().numpy().reshape(shape), value.cpu().numpy(), index.cpu().numpy(), invalid, launched


def check(dev, labels, sources, cost=None, want=None, **kw):
    """The C ABI against the relaxation oracle (and "want", an expectation by construction), table included."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    sources = np.asarray(sources, dtype=np.int32)
    oracle = ref.relaxation(labels, sources, cost)
    if want is not None:
        np.testing.assert_array_equal(ref.bits(oracle), ref.bits(np.asarray(want, dtype=np.float32)))
    field, value, index, invalid, launched = run_geodesic(dev, labels, sources, cost, **kw)
    assert field.dtype == np.float32
    np.testing.assert_array_equal(ref.bits(field), ref.bits(oracle))
    want_value, want_index = ref.farthest(labels, sources, oracle)
    np.testing.assert_array_equal(ref.bits(value), ref.bits(want_value))
    np.testing.assert_array_equal(index, want_index)
    assert invalid == ref.valid_sources(labels, sources)[1]
    return oracle, launched


def index_of(shape, v):
    return int(np.ravel_multi_index(v, shape))


# ---- 1. lines --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 31, 32, 33, 65, 200])
def test_lines_along_x(dev, w):
    shape = (3, 3, w)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 1, :] = 1
    for x in sorted({0, w // 2, w - 1}):      # towards higher and lower indices, across x = 32 | 33 ...
        want = np.zeros(shape, dtype=np.float32)
        want[1, 1, :] = np.abs(np.arange(w) - x)
        check(dev, labels, [-1, index_of(shape, (1, 1, x))], want=want)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("length", [7, 8, 9, 17])
def test_lines_along_z_and_y(dev, axis, length):
    shape = [3, 3, 5]
    shape[axis] = length
    labels = np.zeros(shape, dtype=np.int32)
    line = [1, 1, 2]
    line[axis] = slice(None)
    labels[tuple(line)] = 1
    for p in sorted({0, length // 2, length - 1}):
        at = [1, 1, 2]
        at[axis] = p
        want = np.zeros(shape, dtype=np.float32)
        want[tuple(line)] = np.abs(np.arange(length) - p)
        check(dev, labels, [-1, index_of(shape, at)], want=want)


# ---- 2. diagonals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [0, 24])
def test_diagonals_through_tile_corners(dev, x0):
    """(i, i, 24 + i) steps from tile (0, 0, 0) into tile (1, 1, 1) at i = 8: only the corner neighbour holds the
    next voxel, and a kernel that flags face neighbours alone stops there."""
    shape = (20, 20, 40)
    n = 20 if x0 == 0 else 16
    i = np.arange(n)
    labels = np.zeros(shape, dtype=np.int32)
    labels[i, i, x0 + i] = 1
    if x0:
        assert (7 // 8, 7 // 8, 31 // 32) == (0, 0, 0) and (8 // 8, 8 // 8, 32 // 32) == (1, 1, 1)
    sums, total = [], np.float32(0)
    for _ in range(n):
        sums.append(total)
        total = np.float32(total + ref.SQRT3)      # the repeated float32 sum of 0x3FDDB3D7
    for start in (0, n - 1):
        want = np.zeros(shape, dtype=np.float32)
        want[i, i, x0 + i] = np.array(sums if start == 0 else sums[::-1], dtype=np.float32)
        check(dev, labels, [-1, index_of(shape, (start, start, x0 + start))], want=want)


# ---- 3. a serpentine that re-enters tiles --------------------------------------------------------------------
_SERPENTINE = []


def serpentine_case():
    if not _SERPENTINE:
        labels = ref.serpentine()
        sources = np.array([-1, index_of(labels.shape, (3, 0, 0))], dtype=np.int32)
        oracle = ref.relaxation(labels, sources)
        for a in (labels, sources, oracle):
            a.setflags(write=False)
        _SERPENTINE.append((labels, sources, oracle))
    return _SERPENTINE[0]


@pytest.mark.parametrize("sweeps_per_read", [1, 3, 32])
def test_a_serpentine_with_any_number_of_sweeps_per_read(dev, sweeps_per_read):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, oracle = serpentine_case()
    assert labels.shape == (16, 16, 64) and oracle.max() > 8 * 60      # eight rows, one after another
    stats = {}
    got = inference.geodesic_field(labels.copy(), sources.copy(), sweeps_per_read=sweeps_per_read, stats=stats)
    np.testing.assert_array_equal(ref.bits(got), ref.bits(oracle))
    print(f"serpentine: sweeps_per_read={sweeps_per_read} -> {stats}")
    assert stats["sweeps"] == sweeps_per_read * (stats["reads"] - 1) and stats["tiles_flagged"][-1] == 0
    assert stats["sweeps"] > 3      # every row crosses x = 31 | 32: the two tiles take turns
    if sweeps_per_read == 1:
        assert 8 <= stats["sweeps"] <= 40 and all(stats["tiles_flagged"][:-1])
        with pytest.raises(RuntimeError, match="not converged after 3 sweeps"):
            inference.geodesic_field(labels.copy(), sources.copy(), sweeps_per_read=2, max_sweeps=3)
        inference.geodesic_field(labels.copy(), sources.copy(), sweeps_per_read=7, max_sweeps=stats["sweeps"])


# ---- 4. labels next to each other, in pieces, outside 1..K; sources missing and invalid --------------------
def test_two_labels_touching_along_a_plane(dev):
    shape = (10, 12, 40)
    labels = np.ones(shape, dtype=np.int32)
    labels[:, 6:, :] = 2
    oracle, _ = check(dev, labels, [-1, 0, -1])      # label 2 has no source: nothing leaks into it
    assert np.isposinf(oracle[labels == 2]).all() and np.isfinite(oracle[labels == 1]).all()
    oracle, _ = check(dev, labels, [-1, 0, index_of(shape, (9, 11, 39))])
    assert np.isfinite(oracle).all() and oracle[0, 5, 0] == 5 and oracle[9, 6, 39] == 5


def test_one_id_in_two_pieces(dev):
    labels = np.zeros((9, 9, 70), dtype=np.int32)
    labels[2:5, 2:5, 3:30] = 3
    labels[2:5, 2:5, 31:66] = 3      # x = 30 is background: two voxels apart
    oracle, _ = check(dev, labels, [-1, -1, -1, index_of(labels.shape, (3, 3, 10))])
    assert np.isposinf(oracle[:, :, 31:][labels[:, :, 31:] == 3]).all() and np.isfinite(oracle[:, :, :30]).all()


def test_labels_above_n_labels_and_negative_labels(dev):
    rng = np.random.default_rng(5)
    labels = ref.blobs(rng, (12, 14, 40), 4, fill=0.9)
    labels[rng.random(labels.shape) < 0.05] = -2
    labels[rng.random(labels.shape) < 0.05] = 2**31 - 1
    sources = ref.first_voxels(labels, 2)      # K = 2: labels 3 and 4 are above it
    oracle, _ = check(dev, labels, sources)
    assert np.isposinf(oracle[labels > 2]).all() and (oracle[labels < 0] == 0).all()
    assert np.isfinite(oracle[labels == 1]).any()


def test_sources_minus_one_and_no_labels(dev):
    rng = np.random.default_rng(6)
    labels = ref.blobs(rng, (9, 17, 33), 3)
    oracle, launched = check(dev, labels, [-1, -1, -1, -1])
    assert launched == 0 and np.isposinf(oracle[labels > 0]).all()
    check(dev, labels, [5])      # K = 0: every label is above it, row 0 is ignored


def test_an_invalid_source_row(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels = np.zeros((4, 9, 40), dtype=np.int32)
    labels[1, 2:7, 3:37] = 1
    labels[2, 2:7, 3:37] = 2
    good = index_of(labels.shape, (1, 3, 5))
    for bad in (index_of(labels.shape, (1, 3, 6)), 0, labels.size, -2, 2**31 - 1):      # label 1, background, outside
        sources = np.array([-1, good, bad], dtype=np.int32)
        oracle, _ = check(dev, labels, sources)      # counted, and label 2 is treated as having no source
        assert np.isposinf(oracle[labels == 2]).all() and np.isfinite(oracle[labels == 1]).all()
        with pytest.raises(ValueError, match="1 row.s. of sources name no voxel of their label"):
            inference.geodesic_field(labels, sources)
    assert run_geodesic(dev, labels, [7, labels.size, -5])[3] == 2
    inference.geodesic_field(labels, np.array([12345, good, -1], dtype=np.int32))      # row 0 is ignored


def test_degenerate_volumes(dev):
    check(dev, np.zeros((5, 9, 33), dtype=np.int32), [-1, -1], want=np.zeros((5, 9, 33)))
    check(dev, np.zeros((1, 1, 1), dtype=np.int32), [-1], want=np.zeros((1, 1, 1)))
    check(dev, np.ones((1, 1, 1), dtype=np.int32), [-1, 0], want=np.zeros((1, 1, 1)))
    check(dev, np.ones((1, 1, 1), dtype=np.int32), [-1, -1], want=np.full((1, 1, 1), np.inf))
    check(dev, np.full((1, 1, 1), -1, dtype=np.int32), [-1, -1], want=np.zeros((1, 1, 1)))


# ---- 5. seeded volumes -------------------------------------------------------------------------------------
# every third volume has a shape picked for the tiles: full size, one past a tile edge on every axis, one tile
# exactly, single-voxel axes; the others draw theirs up to 24 x 24 x 40
FORCED_SHAPES = {0: (24, 24, 40), 3: (17, 9, 33), 6: (9, 17, 40), 9: (24, 24, 40), 12: (8, 8, 32), 15: (16, 16, 33),
                 18: (24, 9, 40), 21: (24, 24, 40), 24: (1, 24, 40), 27: (24, 24, 1)}


def seeded(seed):
    return ref.seeded_case(100 + seed, max_shape=(24, 24, 40), max_labels=6, shape=FORCED_SHAPES.get(seed))


@pytest.mark.parametrize("seed", list(range(30)))
def test_seeded_volume(dev, seed):
    labels, sources, cost = seeded(seed)
    assert (cost is None) == (seed % 2 == 0) and 1 <= len(sources) - 1 <= 6
    assert all(a <= b for a, b in zip(labels.shape, (24, 24, 40)))
    check(dev, labels, sources, cost, sweeps_per_call=1 + seed % 3)


def test_cost_mode_with_every_special_value(dev):
    rng = np.random.default_rng(17)
    labels = np.ones((10, 11, 45), dtype=np.int32)
    labels[:, :, 20] = 2
    cost = ref.random_cost(rng, labels.shape)
    zero = cost == 0
    assert zero.any() and np.signbit(cost[zero]).any() and np.isnan(cost).any() and np.isposinf(cost).any()
    assert (cost < 0).any()
    sources = [-1, index_of(labels.shape, (4, 5, 2)), index_of(labels.shape, (0, 0, 20))]
    cost[4, 5, 2] = np.nan      # a source that cannot be entered still starts at 0
    oracle, _ = check(dev, labels, sources, cost)
    assert oracle[4, 5, 2] == 0 and np.isposinf(oracle[(labels > 0) & ~(cost >= 0)]).sum() >= 100
    assert np.isfinite(oracle[:, :, 21:]).sum() == 0      # label 1 beyond the wall of label 2


# ---- 6. the farthest table ---------------------------------------------------------------------------------
def test_the_farthest_table(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    shape = (6, 9, 70)
    labels = np.zeros(shape, dtype=np.int32)
    labels[2, 4, 3:68] = 1           # source in the middle: both ends tie at 32
    labels[4, 1:8, 10] = 2           # reachable piece of label 2 ...
    labels[4, 1:8, 50] = 2           # ... and one that is not
    labels[0, 0, 0:5] = 3            # present, without a source
    sources = np.array([-1, index_of(shape, (2, 4, 35)), index_of(shape, (4, 1, 10)), -1, -1], dtype=np.int32)   # 4 absent
    oracle, _ = check(dev, labels, sources)
    value, index = ref.farthest(labels, sources, oracle)
    assert value.tolist() == [0, 32, 6, 0, 0]
    assert index.tolist() == [-1, index_of(shape, (2, 4, 3)), index_of(shape, (4, 7, 10)), -1, -1]
    field, far_value, far_index = inference.geodesic_field(labels, sources, return_farthest=True)
    np.testing.assert_array_equal(ref.bits(field), ref.bits(oracle))
    assert far_value.dtype == np.float32 and far_index.dtype == np.int32
    np.testing.assert_array_equal(far_value, value)
    np.testing.assert_array_equal(far_index, index)
    t = torch.from_numpy(labels).to(dev)
    out = inference.geodesic_field(t, torch.from_numpy(sources).to(dev), return_farthest=True,
                                   return_device_tensors=True, n_labels=4)
    assert all(isinstance(o, torch.Tensor) and o.device == t.device for o in out)
    np.testing.assert_array_equal(ref.bits(out[0].cpu().numpy()), ref.bits(oracle))
    np.testing.assert_array_equal(out[2].cpu().numpy(), index)
    alone = inference.geodesic_field(t, torch.from_numpy(sources).to(dev), return_device_tensors=True)
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.float32 and tuple(alone.shape) == shape


# ---- 7. more tiles than one launch covers ------------------------------------------------------------------
def test_launch_cap(dev):
    """
    (262152, 9, 9) has 32769 x 2 x 1 = 65538 tiles: the sweep launches 65536 workgroups and strides. Three
    blobs of at most 200 voxels: at z = 0, straddling z = 262144 (tiles 65536 and 65537 lie behind it) and at
    the far end; each is compared on its own crop, the rest of the volume is background and must be 0.
    """
    from aind_exaspim_neuron_segmentation_amd import inference

    shape = (262152, 9, 9)
    tiles_zyx = tuple(-(-s // t) for s, t in zip(shape, TILE))
    assert int(np.prod(tiles_zyx)) == 65538 > 65536
    rng = np.random.default_rng(41)
    labels = np.zeros(shape, dtype=np.int32)
    spans = {1: (0, 6), 2: (262138, 262147), 3: (262148, 262152)}
    sources = np.full(4, -1, dtype=np.int32)
    for label, (z0, z1) in spans.items():
        block = rng.random((z1 - z0, 9, 9)) < 0.2
        block[:, 4, 4] = True      # a spine from the source through every plane of the blob
        labels[z0:z1][block] = label
        sources[label] = index_of(shape, (z0, 4, 4))
        assert block.sum() <= 200
    stats = {}
    field, far_value, far_index = inference.geodesic_field(labels, sources, return_farthest=True, sweeps_per_read=4,
                                                           stats=stats)
    print(f"launch cap: {stats}")
    assert stats["sweeps"] <= 16      # no label spans the volume
    assert (field[labels == 0] == 0).all()
    assert field[262146, 4, 4] == 8 and field[262151, 4, 4] == 3      # behind tile 65536, and the last plane
    for a, b, rows in ((0, 8, (1,)), (262130, 262152, (2, 3))):      # crops that hold whole labels
        crop = labels[a:b]
        local = np.full(4, -1, dtype=np.int32)
        for row in rows:
            local[row] = sources[row] - a * 81
        want = ref.relaxation(crop, local)
        np.testing.assert_array_equal(ref.bits(field[a:b]), ref.bits(want))
        value, index = ref.farthest(crop, local, want)
        for row in rows:
            assert far_value[row] == value[row] and far_index[row] == index[row] + a * 81 and value[row] >= 3


# ---- 8. determinism ----------------------------------------------------------------------------------------
def test_runs_repeat(dev):
    labels = ref.blobs(np.random.default_rng(3), (24, 24, 40), 5)
    sources = ref.first_voxels(labels, 5)
    first = run_geodesic(dev, labels, sources)
    again = run_geodesic(dev, labels, sources, sweeps_per_call=1)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    assert first[2].tobytes() == again[2].tobytes()
    cost = ref.random_cost(np.random.default_rng(4), labels.shape)
    assert run_geodesic(dev, labels, sources, cost)[0].tobytes() == run_geodesic(dev, labels, sources, cost)[0].tobytes()


# ---- 9. refusals, before anything is launched --------------------------------------------------------------
def test_refusals_leave_every_output_alone(dev):
    lib = _native.lib()
    shape = (5, 9, 36)
    n = int(np.prod(shape))
    host = ref.blobs(np.random.default_rng(89), shape, 2)
    host_sources = ref.first_voxels(host, 2)
    labels = torch.from_numpy(host).to(dev)
    sources = torch.from_numpy(host_sources).to(dev)
    cost = torch.ones(shape, dtype=torch.float32, device=dev)
    need = lib.exaspim_geodesic_workspace_bytes(_native.int3(shape))
    far_need = lib.exaspim_geodesic_farthest_workspace_bytes(2)
    field = torch.full((n,), -1234567.0, dtype=torch.float32, device=dev)
    state = torch.full((2,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    value = torch.full((3,), -5.5, dtype=torch.float32, device=dev)
    index = torch.full((3,), -77, dtype=torch.int32, device=dev)
    far_ws = torch.full((far_need,), 0xFF, dtype=torch.uint8, device=dev)
    dims = _native.int3(shape)
    calls = {
        "begin": (lib.exaspim_geodesic_begin, ["labels", "dims", "sources", "k", "field", "state", "ws", "need", "stream"],
                  lambda: [labels.data_ptr(), dims, sources.data_ptr(), 2, field.data_ptr(), state.data_ptr(),
                           ws.data_ptr(), need, None]),
        "sweeps": (lib.exaspim_geodesic_sweeps,
                   ["labels", "cost", "dims", "k", "field", "sweeps", "state", "ws", "need", "stream"],
                   lambda: [labels.data_ptr(), cost.data_ptr(), dims, 2, field.data_ptr(), 3, state.data_ptr(),
                            ws.data_ptr(), need, None]),
        "farthest": (lib.exaspim_geodesic_farthest,
                     ["labels", "field", "dims", "k", "value", "index", "ws", "need", "stream"],
                     lambda: [labels.data_ptr(), field.data_ptr(), dims, 2, value.data_ptr(), index.data_ptr(),
                              far_ws.data_ptr(), far_need, None]),
    }

    def call(which, **changes):
        fn, names, make = calls[which]
        args = make()
        for name, new in changes.items():
            args[names.index(name)] = new
        rc = fn(*args)
        torch.cuda.synchronize()
        return rc

    def refused(which, code, what, **changes):
        assert call(which, **changes) == code, (which, changes, _native.last_error())
        assert what in _native.last_error(), (which, changes, _native.last_error())
        assert (field == -1234567.0).all() and (state == -7654321).all() and (ws == 0xFF).all(), (which, changes)
        assert (value == -5.5).all() and (index == -77).all() and (far_ws == 0xFF).all(), (which, changes)
        np.testing.assert_array_equal(labels.cpu().numpy(), host)

    for which, pointers in (("begin", ("labels", "sources", "field", "state", "ws")),
                            ("sweeps", ("labels", "field", "state", "ws")),
                            ("farthest", ("labels", "field", "value", "index", "ws"))):
        for name in pointers:
            refused(which, -1, "NULL", **{name: None})
        refused(which, -1, "dims", dims=_native.int3((5, 0, 36)))
        refused(which, -1, "dims", dims=_native.int3((5, -9, 36)))
        refused(which, -1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
        refused(which, -1, "n_labels", k=-1)
        refused(which, -1, "misaligned", labels=labels.data_ptr() + 2)
        refused(which, -1, "misaligned", ws=(ws if which != "farthest" else far_ws).data_ptr() + 8)
        refused(which, -3, "workspace", need=(need if which != "farthest" else far_need) - 1)
        refused(which, -3, "workspace", need=0)
    refused("begin", -1, "misaligned", field=field.data_ptr() + 1)
    refused("begin", -1, "misaligned", sources=sources.data_ptr() + 2)
    refused("sweeps", -1, "misaligned", cost=cost.data_ptr() + 2)
    refused("sweeps", -1, "misaligned", state=state.data_ptr() + 1)
    refused("sweeps", -1, "sweeps", sweeps=0)
    refused("sweeps", -1, "sweeps", sweeps=-3)
    refused("farthest", -1, "misaligned", value=value.data_ptr() + 2)

    # the same buffers serve a sound run
    assert call("begin") == 0, _native.last_error()
    seeing = set()      # the tiles that hold a source or see it in their halo
    for s in host_sources[1:]:
        v = np.unravel_index(s, shape)
        for o in [(0, 0, 0)] + ref.OFFSETS:
            u = tuple(a + b for a, b in zip(v, o))
            if all(0 <= a < b for a, b in zip(u, shape)):
                seeing.add(tuple(a // b for a, b in zip(u, TILE)))
    assert state.tolist() == [len(seeing), 0]
    for _ in range(64):
        assert call("sweeps", cost=None) == 0, _native.last_error()
        if state.tolist()[0] == 0:
            break
    assert state.tolist() == [0, 0]
    assert call("farthest") == 0, _native.last_error()
    want = ref.relaxation(host, host_sources)
    np.testing.assert_array_equal(ref.bits(field.cpu().numpy().reshape(shape)), ref.bits(want))
    want_value, want_index = ref.farthest(host, host_sources, want)
    np.testing.assert_array_equal(value.cpu().numpy(), want_value)
    np.testing.assert_array_equal(index.cpu().numpy(), want_index)
    before = field.clone()
    assert call("sweeps", cost=None) == 0 and state.tolist() == [0, 0]      # converged: further sweeps do nothing
    assert torch.equal(before, field)


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    host = np.full((5, 6, 36), 1, dtype=np.int32)
    src = np.array([-1, 0], dtype=np.int32)
    t, s = torch.from_numpy(host).to(dev), torch.from_numpy(src).to(dev)
    for bad in (host.astype(np.int64), t.long(), t.float()):
        with pytest.raises(TypeError, match="labels must be int32"):
            inference.geodesic_field(bad, s if isinstance(bad, torch.Tensor) else src)
    with pytest.raises(TypeError, match="sources must be int32"):
        inference.geodesic_field(t, s.long())
    with pytest.raises(ValueError, match="sources must be"):
        inference.geodesic_field(t, s[None])
    with pytest.raises(TypeError, match="cost must be float32"):
        inference.geodesic_field(t, s, cost=t)
    with pytest.raises(ValueError, match="cost must have the labels' shape"):
        inference.geodesic_field(t, s, cost=torch.ones((5, 6, 35), device=dev))
    with pytest.raises(RuntimeError, match="cost must be on the labels' device"):
        inference.geodesic_field(t, s, cost=torch.ones((5, 6, 36)))
    with pytest.raises(RuntimeError, match="sources must be on the labels' device"):
        inference.geodesic_field(t, torch.from_numpy(src.copy()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.geodesic_field(torch.from_numpy(host.copy()), torch.from_numpy(src.copy()))
    with pytest.raises(ValueError, match="sweeps_per_read"):
        inference.geodesic_field(t, s, sweeps_per_read=0)
    strided = t.permute(2, 1, 0)      # a view that is not contiguous is copied
    z, y, x = np.indices((36, 6, 5))
    got = inference.geodesic_field(strided, s, cost=torch.ones((36, 6, 5), device=dev))
    np.testing.assert_array_equal(got, np.maximum.reduce([z, y, x]).astype(np.float32))


# ---- 10. the chain -----------------------------------------------------------------------------------------
def test_from_agglomerate_affinities_to_the_distance_from_root_field_on_the_device(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    rng = np.random.default_rng(7)
    shape = (40, 48, 64)
    z, y, x = np.indices(shape)
    ball = ((z - 20) ** 2 + (y - 26) ** 2 + (x - 44) ** 2) <= 81      # a soma of radius 9
    inside = (((y - 10) ** 2 + (x - 14) ** 2) <= 25) | ball           # and a neurite along z
    carved = [(20, 26, 44), (20, 26, 45), (21, 26, 44)]               # background voxels at the soma's centre
    for v in carved:
        inside[v] = False
    aff = np.full((3,) + shape, 0.05, dtype=np.float32)
    aff[0, :-1][inside[:-1] & inside[1:]] = 0.9
    aff[1, :, :-1][inside[:, :-1] & inside[:, 1:]] = 0.9
    aff[2, :, :, :-1][inside[:, :, :-1] & inside[:, :, 1:]] = 0.9
    aff += rng.random((3,) + shape, dtype=np.float32) * 0.05
    labels = inference.agglomerate_affinities(torch.from_numpy(aff).to(dev), min_segment_size=10,
                                              return_device_tensor=True)
    host = labels.cpu().numpy()
    assert host.max() == 2

    # nothing leaves the device in between
    filled, _ = inference._fill_holes_on_device(labels)
    first = inference.segment_table(filled, n_labels=2, return_device_tensors=True)[3]      # each label's first voxel
    _, _, roots = inference.geodesic_field(filled, first, return_farthest=True, return_device_tensors=True)
    daf, far_value, far_index = inference.geodesic_field(filled, roots, return_farthest=True,
                                                         return_device_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.device == labels.device for t in (first, roots, daf, far_value))

    want_labels, _ = holes_ref.by_components(host)
    np.testing.assert_array_equal(filled.cpu().numpy(), want_labels)
    want_first = ref.first_voxels(want_labels, 2)
    np.testing.assert_array_equal(first.cpu().numpy(), want_first)
    _, want_roots = ref.farthest(want_labels, want_first, ref.relaxation(want_labels, want_first))
    np.testing.assert_array_equal(roots.cpu().numpy(), want_roots)
    want_daf = ref.relaxation(want_labels, want_roots)
    np.testing.assert_array_equal(ref.bits(daf.cpu().numpy()), ref.bits(want_daf))
    want_value, want_index = ref.farthest(want_labels, want_roots, want_daf)
    np.testing.assert_array_equal(far_value.cpu().numpy(), want_value)
    np.testing.assert_array_equal(far_index.cpu().numpy(), want_index)
    neurite = int(host[0, 10, 14])
    assert want_value[neurite] >= 39 and np.isfinite(want_daf).all()      # from one end of the neurite to the other
    # soma roots: the maximum of the distance-to-boundary field as the source
    dbf = inference.distance_to_boundary(filled, return_device_tensor=True)
    soma_roots = inference.segment_table(filled, dbf, n_labels=2, return_device_tensors=True)[3]
    from_soma = inference.geodesic_field(filled, soma_roots, return_device_tensors=True)
    np.testing.assert_array_equal(ref.bits(from_soma.cpu().numpy()),
                                  ref.bits(ref.relaxation(want_labels, soma_roots.cpu().numpy())))
