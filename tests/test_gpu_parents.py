"""
exaspim_geodesic_parents_begin / _sweeps / _finish, exaspim_trace_paths and inference.geodesic_parents /
trace_paths on the GPU (-m gpu). Parents, hops and paths are compared with array_equal on int32 against the
Jacobi oracle of tests/parents_ref.py (tests/test_parents_ref_cpu.py holds it to a breadth-first search): lines
along every axis across the tile edges, diagonals through tile corners, a serpentine that re-enters tiles, the
plateaus where an absorbed cost ties neighbouring voxels, touching labels, an id in two pieces, labels outside
1..K, missing and invalid sources, a field of another cost, degenerate volumes, seeded volumes in both modes, a
volume with more tiles than one capped launch, determinism, every refusal, the paths, and the chain from
agglomerate_affinities to the paths on the device. Every run through the C ABI writes into buffers pre-filled
with 0xFF bytes between guard words that must not change. Nothing here provokes a fault: every refused call is
rejected on the host before a launch, and the walk of a spoiled parents array is bounded and range-checked.
"""

import numpy as np
import pytest
import torch

import geodesic_ref as ref
import holes_ref
import parents_ref as pref
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


def run_parents(dev, labels, sources, field, cost=None, sweeps_per_call=4, limit=4096):
    """
    begin, sweeps until state[0] == 0, finish: through the C ABI into guarded, poisoned buffers.
    Returns (parents, hops, orphans, invalid rows, sweeps launched).
    """
    lib = _native.lib()
    labels = np.array(labels, dtype=np.int32)
    sources = np.array(sources, dtype=np.int32)
    field = np.array(field, dtype=np.float32)
    shape, k = labels.shape, len(sources) - 1
    n = int(np.prod(shape))
    dims = _native.int3(shape)
    lab = torch.from_numpy(labels).to(dev)
    src = torch.from_numpy(sources).to(dev)
    fld = torch.from_numpy(field).to(dev)
    cst = None if cost is None else torch.from_numpy(np.array(cost, dtype=np.float32)).to(dev)
    cost_ptr = None if cst is None else cst.data_ptr()
    need = lib.exaspim_geodesic_workspace_bytes(dims)
    assert need >= 32, _native.last_error()
    hops_full, hops = guarded(dev, n, torch.int32)
    parents_full, parents = guarded(dev, n, torch.int32)
    state_full, state = guarded(dev, 3, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    rc = lib.exaspim_geodesic_parents_begin(lab.data_ptr(), dims, src.data_ptr(), k, fld.data_ptr(), hops.data_ptr(),
                                            state.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, _native.last_error()
    flagged, invalid = state.cpu().tolist()[:2]
    launched = 0
    while flagged:
        assert launched < limit, "no convergence"
        rc = lib.exaspim_geodesic_parents_sweeps(lab.data_ptr(), cost_ptr, fld.data_ptr(), dims, k, hops.data_ptr(),
                                                 sweeps_per_call, state.data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        launched += sweeps_per_call
        flagged, still_invalid = state.cpu().tolist()[:2]
        assert still_invalid == invalid
    rc = lib.exaspim_geodesic_parents_finish(lab.data_ptr(), cost_ptr, fld.data_ptr(), hops.data_ptr(), dims, k,
                                             parents.data_ptr(), state.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert state.cpu().tolist()[:2] == [0, invalid]
    orphans = int(state.cpu()[2])
    assert intact(hops_full, n, torch.int32) and intact(parents_full, n, torch.int32)
    assert intact(state_full, 3, torch.int32) and intact(ws_full, need, torch.uint8)
    np.testing.assert_array_equal(lab.cpu().numpy(), labels)      # the inputs are only read
    np.testing.assert_array_equal(src.cpu().numpy(), sources)
    assert fld.cpu().numpy().tobytes() == field.tobytes()
    return parents.cpu().numpy().reshape(shape), hops.cpu().numpy().reshape(shape), orphans, invalid, launched


def run_trace(dev, parents, hops, targets, offsets=None, capacity=None):
    """exaspim_trace_paths into guarded buffers: (paths, offsets, state). Offsets default to the sound ones."""
    lib = _native.lib()
    parents = np.array(parents, dtype=np.int32)      # copies: a shared case is read-only
    hops = np.array(hops, dtype=np.int32)
    targets = np.array(targets, dtype=np.int32)
    if offsets is None:
        offsets = np.zeros(len(targets) + 1, dtype=np.int64)
        np.cumsum(hops.reshape(-1)[targets].astype(np.int64) + 1, out=offsets[1:])
    offsets = np.array(offsets, dtype=np.int64)
    total = int(offsets[-1]) if capacity is None else capacity
    par, hop = torch.from_numpy(parents).to(dev), torch.from_numpy(hops).to(dev)
    tgt, off = torch.from_numpy(targets).to(dev), torch.from_numpy(offsets).to(dev)
    paths_full, paths = guarded(dev, total, torch.int32)
    state_full, state = guarded(dev, 2, torch.int32)
    rc = lib.exaspim_trace_paths(par.data_ptr(), hop.data_ptr(), _native.int3(parents.shape),
                                 tgt.data_ptr() if len(targets) else None, len(targets), off.data_ptr(),
                                 paths.data_ptr() if total else None, total, state.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(paths_full, total, torch.int32) and intact(state_full, 2, torch.int32)
    np.testing.assert_array_equal(par.cpu().numpy(), parents)
    return paths.cpu().numpy(), offsets, state.cpu().tolist()


def check(dev, labels, sources, cost=None, field=None, orphans=0, trace=True, **kw):
    """The C ABI against the Jacobi oracle on the oracle's own field; then the paths of some targets."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    sources = np.asarray(sources, dtype=np.int32)
    if field is None:
        field = ref.relaxation(labels, sources, cost)
    want_parents, want_hops, want_orphans, want_invalid = pref.jacobi(labels, sources, field, cost)
    parents, hops, got_orphans, invalid, launched = run_parents(dev, labels, sources, field, cost, **kw)
    assert parents.dtype == np.int32 and hops.dtype == np.int32
    np.testing.assert_array_equal(hops, want_hops)
    np.testing.assert_array_equal(parents, want_parents)
    assert (got_orphans, invalid) == (want_orphans, want_invalid)
    if orphans is not None:
        assert got_orphans == orphans
    if trace and got_orphans == 0:
        reached = np.nonzero(hops.reshape(-1) >= 0)[0]
        if reached.size:
            far = reached[np.argsort(-hops.reshape(-1)[reached], kind="stable")][:8]
            check_paths(dev, labels.shape, parents, hops, np.concatenate([far, reached[:4]]).astype(np.int32))
    return want_parents, want_hops, field, launched


def check_paths(dev, shape, parents, hops, targets):
    """Positions equal hops, neighbours are adjacent, every path ends at its target and starts at a source."""
    paths, offsets, state = run_trace(dev, parents, hops, targets)
    assert state == [0, 0]
    want, want_offsets = pref.paths(parents, hops, targets)
    np.testing.assert_array_equal(offsets, want_offsets)
    np.testing.assert_array_equal(paths, want)
    flat_h = hops.reshape(-1)
    for i, t in enumerate(targets):
        row = paths[offsets[i]:offsets[i + 1]]
        assert row[-1] == t and flat_h[row[0]] == 0
        np.testing.assert_array_equal(flat_h[row], np.arange(len(row)))
        coords = np.stack(np.unravel_index(row, shape), axis=1)
        if len(row) > 1:
            assert np.abs(np.diff(coords, axis=0)).max(axis=1).tolist() == [1] * (len(row) - 1)
    return paths, offsets


def index_of(shape, v):
    return int(np.ravel_multi_index(v, shape))


# ---- 1. lines --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 31, 32, 33, 64, 65, 200])
def test_lines_along_x(dev, w):
    shape = (3, 3, w)
    labels = np.zeros(shape, dtype=np.int32)
    labels[1, 1, :] = 1
    for x in sorted({0, w // 2, w - 1}):      # towards higher and lower indices, across x = 31 | 32 ...
        parents, hops, _, _ = check(dev, labels, [-1, index_of(shape, (1, 1, x))])
        np.testing.assert_array_equal(hops[1, 1], np.abs(np.arange(w) - x))
        step = np.sign(x - np.arange(w))
        np.testing.assert_array_equal(parents[1, 1], index_of(shape, (1, 1, 0)) + np.arange(w) + step)


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
        _, hops, _, _ = check(dev, labels, [-1, index_of(shape, at)])
        np.testing.assert_array_equal(hops[tuple(line)], np.abs(np.arange(length) - p))


# ---- 2. diagonals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [0, 24])
def test_diagonals_through_tile_corners(dev, x0):
    """(i, i, 24 + i) steps from tile (0, 0, 0) into tile (1, 1, 1) at i = 8: only the corner neighbour holds it."""
    shape = (20, 20, 40)
    n = 20 if x0 == 0 else 16
    i = np.arange(n)
    labels = np.zeros(shape, dtype=np.int32)
    labels[i, i, x0 + i] = 1
    for start in (0, n - 1):
        _, hops, _, _ = check(dev, labels, [-1, index_of(shape, (start, start, x0 + start))])
        np.testing.assert_array_equal(hops[i, i, x0 + i], np.abs(i - start))


# ---- 3. a serpentine that re-enters tiles --------------------------------------------------------------------
_SERPENTINE = []


def serpentine_case():
    if not _SERPENTINE:
        labels = ref.serpentine()
        sources = np.array([-1, index_of(labels.shape, (3, 0, 0))], dtype=np.int32)
        field = ref.relaxation(labels, sources)
        parents, hops, orphans, invalid = pref.jacobi(labels, sources, field)
        assert (orphans, invalid) == (0, 0)
        for a in (labels, sources, field, parents, hops):
            a.setflags(write=False)
        _SERPENTINE.append((labels, sources, field, parents, hops))
    return _SERPENTINE[0]


@pytest.mark.parametrize("sweeps_per_read", [1, 3, 32])
def test_a_serpentine_with_any_number_of_sweeps_per_read(dev, sweeps_per_read):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, field, want_parents, want_hops = serpentine_case()
    assert labels.shape == (16, 16, 64) and want_hops.max() > 8 * 60      # eight rows, one after another
    stats = {}
    parents, hops = inference.geodesic_parents(labels.copy(), sources.copy(), field=field.copy(), return_hops=True,
                                               sweeps_per_read=sweeps_per_read, stats=stats)
    np.testing.assert_array_equal(hops, want_hops)
    np.testing.assert_array_equal(parents, want_parents)
    print(f"serpentine: sweeps_per_read={sweeps_per_read} -> {stats}")
    assert stats["sweeps"] == sweeps_per_read * (stats["reads"] - 2) and stats["tiles_flagged"][-1] == 0
    assert stats["sweeps"] > 3      # every row crosses x = 31 | 32: the two tiles take turns
    if sweeps_per_read == 1:
        with pytest.raises(RuntimeError, match="not converged after 3 sweeps"):
            inference.geodesic_parents(labels.copy(), sources.copy(), field=field.copy(), sweeps_per_read=2,
                                       max_sweeps=3)


# ---- 4. plateaus: an absorbed cost ties neighbouring voxels ------------------------------------------------
def test_plateau_line(dev):
    """d = 2^25 on x = 0 .. 68: both x - 1 -> x and x + 1 -> x are tight, and only hops tell the way."""
    labels, sources, cost = pref.plateau_line()
    parents, hops, field, _ = check(dev, labels, sources, cost)
    n = labels.shape[2]
    assert n == 70 and pref.plateau_count(parents, field) >= 1
    x = np.arange(n - 1)
    np.testing.assert_array_equal(parents[1, 1, :n - 1], index_of(labels.shape, (1, 1, 0)) + x + 1)      # towards +x
    np.testing.assert_array_equal(hops[1, 1], n - 1 - np.arange(n))


def test_plateau_slab(dev):
    labels, sources, cost = pref.plateau_slab()
    parents, hops, field, _ = check(dev, labels, sources, cost)
    assert labels.shape == (3, 12, 40) and pref.plateau_count(parents, field) >= 1
    assert (hops >= 0).all()


# ---- 5. labels next to each other, in pieces, outside 1..K; sources missing and invalid --------------------
def test_two_labels_touching_along_a_plane(dev):
    shape = (10, 12, 40)
    labels = np.ones(shape, dtype=np.int32)
    labels[:, 6:, :] = 2
    _, hops, _, _ = check(dev, labels, [-1, 0, -1])      # label 2 has no source: nothing leaks into it
    assert (hops[labels == 2] == -1).all() and (hops[labels == 1] >= 0).all()
    parents, hops, _, _ = check(dev, labels, [-1, 0, index_of(shape, (9, 11, 39))])
    assert (hops >= 0).all()
    assert (labels.reshape(-1)[parents.reshape(-1)] == labels.reshape(-1)).all()      # no parent across the plane


def test_one_id_in_two_pieces(dev):
    labels = np.zeros((9, 9, 70), dtype=np.int32)
    labels[2:5, 2:5, 3:30] = 3
    labels[2:5, 2:5, 31:66] = 3      # x = 30 is background: two voxels apart
    parents, hops, _, _ = check(dev, labels, [-1, -1, -1, index_of(labels.shape, (3, 3, 10))])
    assert (hops[:, :, 31:] == -1).all() and (parents[:, :, 31:] == -1).all()
    assert (hops[:, :, :30][labels[:, :, :30] == 3] >= 0).all()


def test_labels_above_n_labels_and_negative_labels(dev):
    rng = np.random.default_rng(5)
    labels = ref.blobs(rng, (12, 14, 40), 4, fill=0.9)
    labels[rng.random(labels.shape) < 0.05] = -2
    labels[rng.random(labels.shape) < 0.05] = 2**31 - 1
    sources = ref.first_voxels(labels, 2)      # K = 2: labels 3 and 4 are above it
    parents, hops, _, _ = check(dev, labels, sources)
    assert (hops[(labels > 2) | (labels <= 0)] == -1).all() and (parents[(labels > 2) | (labels <= 0)] == -1).all()
    assert (hops[labels == 1] >= 0).any()


def test_sources_minus_one_and_no_labels(dev):
    rng = np.random.default_rng(6)
    labels = ref.blobs(rng, (9, 17, 33), 3)
    parents, hops, _, launched = check(dev, labels, [-1, -1, -1, -1])
    assert launched == 0 and (hops == -1).all() and (parents == -1).all()
    check(dev, labels, [5])      # K = 0: every label is above it, row 0 is ignored


def test_invalid_rows_and_a_source_whose_field_was_overwritten(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels = np.zeros((4, 9, 40), dtype=np.int32)
    labels[1, 2:7, 3:37] = 1
    labels[2, 2:7, 3:37] = 2
    good = index_of(labels.shape, (1, 3, 5))
    for bad in (index_of(labels.shape, (1, 3, 6)), 0, labels.size, -2, 2**31 - 1):      # label 1, background, outside
        sources = np.array([-1, good, bad], dtype=np.int32)
        field = ref.relaxation(labels, sources)
        _, hops, _, _ = check(dev, labels, sources, field=field)      # counted; label 2 is without a source
        assert (hops[labels == 2] == -1).all() and (hops[labels == 1] >= 0).all()
        with pytest.raises(ValueError, match="1 row.s. of sources name no voxel of their label"):
            inference.geodesic_parents(labels, sources, field=field)
    # a source whose field is not +0.0 counts as invalid; its label's finite voxels are then without hops, and the
    # source itself, which nothing leads to, is an orphan
    sources = np.array([-1, good, index_of(labels.shape, (2, 4, 20))], dtype=np.int32)
    field = ref.relaxation(labels, sources)
    for value in (1.0, -0.0, np.nan):
        spoiled = field.copy()
        spoiled[2, 4, 20] = value
        _, hops, _, _ = check(dev, labels, sources, field=spoiled, orphans=None)
        assert (hops[labels == 2] == -1).all() and (hops[labels == 1] >= 0).all()
        assert run_parents(dev, labels, sources, spoiled)[3] == 1
        with pytest.raises(ValueError, match="1 row.s. of sources name no voxel of their label with a field of 0"):
            inference.geodesic_parents(labels, sources, field=spoiled)


def test_a_field_of_another_cost_makes_orphans(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, cost = ref.seeded_case(101, max_shape=(24, 24, 40), max_labels=6, shape=(17, 9, 33))
    field = ref.relaxation(labels, sources, cost)
    other = np.where(np.isfinite(cost) & (cost > 0), cost * np.float32(1.37), cost).astype(np.float32)
    want = pref.jacobi(labels, sources, field, other)
    assert want[2] > 0      # the oracle sees orphans
    check(dev, labels, sources, other, field=field, orphans=want[2])
    with pytest.raises(ValueError, match="not the geodesic field of these labels, sources and cost"):
        inference.geodesic_parents(labels, sources, field=field, cost=other)
    with pytest.raises(ValueError, match=f"{pref.jacobi(labels, sources, field)[2]} voxel"):
        inference.geodesic_parents(labels, sources, field=field)      # Euclidean steps on a cost field
    inference.geodesic_parents(labels, sources, field=field, cost=cost)


def test_degenerate_volumes(dev):
    check(dev, np.zeros((5, 9, 33), dtype=np.int32), [-1, -1])
    check(dev, np.zeros((1, 1, 1), dtype=np.int32), [-1])
    parents, hops, _, _ = check(dev, np.ones((1, 1, 1), dtype=np.int32), [-1, 0])
    assert parents.tolist() == [[[0]]] and hops.tolist() == [[[0]]]
    parents, hops, _, _ = check(dev, np.ones((1, 1, 1), dtype=np.int32), [-1, -1])
    assert parents.tolist() == [[[-1]]] and hops.tolist() == [[[-1]]]
    check(dev, np.full((1, 1, 1), -1, dtype=np.int32), [-1, -1])


# ---- 6. seeded volumes -------------------------------------------------------------------------------------
FORCED_SHAPES = {0: (24, 24, 40), 3: (17, 9, 33), 6: (9, 17, 40), 9: (24, 24, 40), 12: (8, 8, 32), 15: (16, 16, 33),
                 18: (24, 9, 40), 21: (24, 24, 40), 24: (1, 24, 40), 27: (24, 24, 1)}


def seeded(seed):
    return ref.seeded_case(100 + seed, max_shape=(24, 24, 40), max_labels=6, shape=FORCED_SHAPES.get(seed))


@pytest.mark.parametrize("seed", list(range(30)))
def test_seeded_volume(dev, seed):
    labels, sources, cost = seeded(seed)      # odd seeds: costs with 0, -0.0, +inf, NaN, negatives, tiny and large
    assert (cost is None) == (seed % 2 == 0) and 1 <= len(sources) - 1 <= 6
    assert all(a <= b for a, b in zip(labels.shape, (24, 24, 40)))
    if seed % 8 == 1:      # a quarter of the cost cases: costs that are absorbed
        rng = np.random.default_rng(7000 + seed)
        with np.errstate(invalid="ignore", over="ignore"):
            scaled = (cost * np.float32(3e7)).astype(np.float32)
        cost = np.where(rng.random(cost.shape) < 0.3, np.float32(1e-3), scaled).astype(np.float32)
    check(dev, labels, sources, cost, sweeps_per_call=1 + seed % 3)


# ---- 7. more tiles than one launch covers ------------------------------------------------------------------
def test_launch_cap(dev):
    """
    (262152, 9, 9) has 32769 x 2 x 1 = 65538 tiles: the sweep launches 65536 workgroups and strides. Three
    blobs of at most 200 voxels: at z = 0, straddling z = 262144 (tiles 65536 and 65537 lie behind it) and at
    the far end; each is compared on its own crop, the rest of the volume is background and must be -1.
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
    parents, hops = inference.geodesic_parents(labels, sources, return_hops=True, sweeps_per_read=4, stats=stats)
    print(f"launch cap: {stats}")
    assert stats["sweeps"] <= 16      # no label spans the volume
    assert (hops[labels == 0] == -1).all() and (parents[labels == 0] == -1).all()
    assert hops[262146, 4, 4] == 8 and hops[262151, 4, 4] == 3      # behind tile 65536, and the last plane
    for a, b, rows in ((0, 8, (1,)), (262130, 262152, (2, 3))):      # crops that hold whole labels
        crop = labels[a:b]
        local = np.full(4, -1, dtype=np.int32)
        for row in rows:
            local[row] = sources[row] - a * 81
        want_parents, want_hops, orphans, invalid = pref.jacobi(crop, local, ref.relaxation(crop, local))
        assert (orphans, invalid) == (0, 0)
        np.testing.assert_array_equal(hops[a:b], want_hops)
        np.testing.assert_array_equal(parents[a:b], np.where(want_parents >= 0, want_parents + a * 81, -1))
    voxels, offsets = inference.trace_paths(parents, hops, np.array([index_of(shape, (262146, 4, 4))], dtype=np.int32))
    assert offsets.tolist() == [0, 9] and voxels[0] == sources[2] and voxels[-1] == index_of(shape, (262146, 4, 4))


# ---- 8. determinism, and field=None ----------------------------------------------------------------------
def test_runs_repeat(dev):
    labels = ref.blobs(np.random.default_rng(3), (24, 24, 40), 5)
    sources = ref.first_voxels(labels, 5)
    field = ref.relaxation(labels, sources)
    first = run_parents(dev, labels, sources, field)
    again = run_parents(dev, labels, sources, field, sweeps_per_call=1)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    cost = ref.random_cost(np.random.default_rng(4), labels.shape)
    field = ref.relaxation(labels, sources, cost)
    first, again = run_parents(dev, labels, sources, field, cost), run_parents(dev, labels, sources, field, cost)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("mode", ["euclid", "cost"])
def test_field_none_equals_a_given_field(dev, mode):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels = ref.blobs(np.random.default_rng(13), (17, 24, 40), 4)
    sources = ref.first_voxels(labels, 4)
    cost = ref.random_cost(np.random.default_rng(14), labels.shape) if mode == "cost" else None
    field = ref.relaxation(labels, sources, cost)
    want_parents, want_hops, orphans, _ = pref.jacobi(labels, sources, field, cost)
    assert orphans == 0
    stats = {}
    alone = inference.geodesic_parents(labels, sources, cost=cost, return_hops=True, stats=stats)
    given = inference.geodesic_parents(labels, sources, cost=cost, field=field, return_hops=True)
    assert "field" in stats and stats["field"]["tiles_flagged"][-1] == 0
    for got in (alone, given):
        np.testing.assert_array_equal(got[0], want_parents)
        np.testing.assert_array_equal(got[1], want_hops)
    t = torch.from_numpy(labels).to(dev)
    out = inference.geodesic_parents(t, torch.from_numpy(sources).to(dev), n_labels=4, return_device_tensors=True,
                                     cost=None if cost is None else torch.from_numpy(cost).to(dev))
    assert isinstance(out, torch.Tensor) and out.dtype == torch.int32 and out.device == t.device
    np.testing.assert_array_equal(out.cpu().numpy(), want_parents)


# ---- 9. refusals, before anything is launched --------------------------------------------------------------
def test_refusals_leave_every_output_alone(dev):
    lib = _native.lib()
    shape = (5, 9, 36)
    n = int(np.prod(shape))
    host = ref.blobs(np.random.default_rng(89), shape, 2)
    host_sources = ref.first_voxels(host, 2)
    host_field = ref.relaxation(host, host_sources)
    labels = torch.from_numpy(host).to(dev)
    sources = torch.from_numpy(host_sources).to(dev)
    field = torch.from_numpy(host_field).to(dev)
    cost = torch.ones(shape, dtype=torch.float32, device=dev)
    need = lib.exaspim_geodesic_workspace_bytes(_native.int3(shape))
    hops = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    parents = torch.full((n,), -2345678, dtype=torch.int32, device=dev)
    state = torch.full((3,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    targets = torch.zeros(4, dtype=torch.int32, device=dev)
    offsets = torch.arange(5, dtype=torch.int64, device=dev)
    paths = torch.full((8,), -3456789, dtype=torch.int32, device=dev)
    dims = _native.int3(shape)
    calls = {
        "begin": (lib.exaspim_geodesic_parents_begin,
                  ["labels", "dims", "sources", "k", "field", "hops", "state", "ws", "need", "stream"],
                  lambda: [labels.data_ptr(), dims, sources.data_ptr(), 2, field.data_ptr(), hops.data_ptr(),
                           state.data_ptr(), ws.data_ptr(), need, None]),
        "sweeps": (lib.exaspim_geodesic_parents_sweeps,
                   ["labels", "cost", "field", "dims", "k", "hops", "sweeps", "state", "ws", "need", "stream"],
                   lambda: [labels.data_ptr(), cost.data_ptr(), field.data_ptr(), dims, 2, hops.data_ptr(), 3,
                            state.data_ptr(), ws.data_ptr(), need, None]),
        "finish": (lib.exaspim_geodesic_parents_finish,
                   ["labels", "cost", "field", "hops", "dims", "k", "parents", "state", "stream"],
                   lambda: [labels.data_ptr(), cost.data_ptr(), field.data_ptr(), hops.data_ptr(), dims, 2,
                            parents.data_ptr(), state.data_ptr(), None]),
        "trace": (lib.exaspim_trace_paths,
                  ["parents", "hops", "dims", "targets", "t", "offsets", "paths", "capacity", "state", "stream"],
                  lambda: [parents.data_ptr(), hops.data_ptr(), dims, targets.data_ptr(), 4, offsets.data_ptr(),
                           paths.data_ptr(), 8, state.data_ptr(), None]),
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
        assert (hops == -1234567).all() and (parents == -2345678).all() and (state == -7654321).all(), (which, changes)
        assert (ws == 0xFF).all() and (paths == -3456789).all(), (which, changes)
        np.testing.assert_array_equal(labels.cpu().numpy(), host)

    for which, pointers in (("begin", ("labels", "sources", "field", "hops", "state", "ws")),
                            ("sweeps", ("labels", "field", "hops", "state", "ws")),
                            ("finish", ("labels", "field", "hops", "parents", "state")),
                            ("trace", ("parents", "hops", "targets", "offsets", "paths", "state"))):
        for name in pointers:
            refused(which, -1, "NULL", **{name: None})
        refused(which, -1, "dims", dims=_native.int3((5, 0, 36)))
        refused(which, -1, "dims", dims=_native.int3((5, -9, 36)))
        refused(which, -1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
        refused(which, -1, "misaligned", hops=hops.data_ptr() + 2)
        refused(which, -1, "misaligned", state=state.data_ptr() + 1)
        if which != "trace":
            refused(which, -1, "n_labels", k=-1)
            refused(which, -1, "misaligned", labels=labels.data_ptr() + 2)
            refused(which, -1, "misaligned", field=field.data_ptr() + 1)
        if which in ("begin", "sweeps"):
            refused(which, -1, "misaligned", ws=ws.data_ptr() + 8)
            refused(which, -3, "workspace", need=need - 1)
            refused(which, -3, "workspace", need=0)
        if which in ("sweeps", "finish"):
            refused(which, -1, "misaligned", cost=cost.data_ptr() + 2)
    refused("begin", -1, "misaligned", sources=sources.data_ptr() + 2)
    refused("sweeps", -1, "sweeps", sweeps=0)
    refused("sweeps", -1, "sweeps", sweeps=-3)
    refused("finish", -1, "misaligned", parents=parents.data_ptr() + 2)
    refused("trace", -1, "n_targets", t=-1)
    refused("trace", -1, "paths_capacity", capacity=-1)
    refused("trace", -1, "misaligned", offsets=offsets.data_ptr() + 4)
    refused("trace", -1, "misaligned", targets=targets.data_ptr() + 2)
    refused("trace", -1, "misaligned", paths=paths.data_ptr() + 1)

    # the same buffers serve a sound run
    assert call("begin") == 0, _native.last_error()
    seeing = set()      # the tiles that hold a source or see it in their halo
    for s in host_sources[1:]:
        v = np.unravel_index(s, shape)
        for o in [(0, 0, 0)] + ref.OFFSETS:
            u = tuple(a + b for a, b in zip(v, o))
            if all(0 <= a < b for a, b in zip(u, shape)):
                seeing.add(tuple(a // b for a, b in zip(u, TILE)))
    assert state.tolist() == [len(seeing), 0, -7654321]
    for _ in range(64):
        assert call("sweeps", cost=None) == 0, _native.last_error()
        if state.tolist()[0] == 0:
            break
    assert state.tolist() == [0, 0, -7654321]
    before = hops.clone()
    assert call("sweeps", cost=None) == 0 and state.tolist()[:2] == [0, 0]      # converged: further sweeps do nothing
    assert torch.equal(before, hops)
    assert call("finish", cost=None) == 0, _native.last_error()
    assert state.tolist() == [0, 0, 0]
    want_parents, want_hops, _, _ = pref.jacobi(host, host_sources, host_field)
    np.testing.assert_array_equal(hops.cpu().numpy().reshape(shape), want_hops)
    np.testing.assert_array_equal(parents.cpu().numpy().reshape(shape), want_parents)


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    host = np.full((5, 6, 36), 1, dtype=np.int32)
    src = np.array([-1, 0], dtype=np.int32)
    t, s = torch.from_numpy(host).to(dev), torch.from_numpy(src).to(dev)
    with pytest.raises(TypeError, match="labels must be int32"):
        inference.geodesic_parents(t.long(), s)
    with pytest.raises(TypeError, match="field must be float32"):
        inference.geodesic_parents(t, s, field=t)
    with pytest.raises(ValueError, match="field must have the labels' shape"):
        inference.geodesic_parents(t, s, field=torch.ones((5, 6, 35), device=dev))
    with pytest.raises(RuntimeError, match="field must be on the labels' device"):
        inference.geodesic_parents(t, s, field=torch.ones((5, 6, 36)))
    with pytest.raises(RuntimeError, match="sources must be on the labels' device"):
        inference.geodesic_parents(t, torch.from_numpy(src.copy()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.geodesic_parents(torch.from_numpy(host.copy()), torch.from_numpy(src.copy()))
    parents, hops = inference.geodesic_parents(t, s, return_hops=True, return_device_tensors=True)
    with pytest.raises(RuntimeError, match="targets must be on the parents' device"):
        inference.trace_paths(parents, hops, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="targets must be int32"):
        inference.trace_paths(parents, hops, torch.zeros(1, dtype=torch.int64, device=dev))
    for bad in (-1, host.size, 2**31 - 1):
        with pytest.raises(ValueError, match="1 target.s. out of range or with hops < 0"):
            inference.trace_paths(parents, hops, np.array([3, bad], dtype=np.int32))


# ---- 10. paths ---------------------------------------------------------------------------------------------
_PATHS = []


def paths_case():
    """A seeded volume, its oracle parents and hops: shared, and left unchanged."""
    if not _PATHS:
        labels, sources, cost = seeded(9)
        field = ref.relaxation(labels, sources, cost)
        parents, hops, orphans, invalid = pref.jacobi(labels, sources, field, cost)
        assert (orphans, invalid) == (0, 0) and (hops >= 0).sum() > 300
        for a in (labels, sources, parents, hops):
            a.setflags(write=False)
        _PATHS.append((labels, sources, parents, hops))
    return _PATHS[0]


def test_trace_no_targets_and_the_source_itself(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, parents, hops = paths_case()
    paths, offsets, state = run_trace(dev, parents, hops, np.zeros(0, dtype=np.int32))
    assert paths.size == 0 and offsets.tolist() == [0] and state == [0, 0]
    voxels, offsets = inference.trace_paths(parents.copy(), hops.copy(), np.zeros(0, dtype=np.int32))
    assert voxels.dtype == np.int32 and voxels.shape == (0,) and offsets.dtype == np.int64 and offsets.tolist() == [0]
    source = int(next(s for s in sources[1:] if s >= 0))
    paths, offsets, state = run_trace(dev, parents, hops, np.array([source], dtype=np.int32))
    assert paths.tolist() == [source] and offsets.tolist() == [0, 1] and state == [0, 0]
    voxels, offsets = inference.trace_paths(parents.copy(), hops.copy(), np.array([source, source], dtype=np.int32))
    assert voxels.tolist() == [source, source] and offsets.tolist() == [0, 1, 2]


def test_trace_300_targets_with_duplicates(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, parents, hops = paths_case()
    reached = np.nonzero(hops.reshape(-1) >= 0)[0]
    targets = np.random.default_rng(21).choice(reached, 300).astype(np.int32)
    targets[150:] = targets[:150][::-1]      # every target twice
    paths, offsets = check_paths(dev, labels.shape, parents, hops, targets)
    voxels, got_offsets = inference.trace_paths(parents.copy(), hops.copy(), targets)
    np.testing.assert_array_equal(voxels, paths)
    np.testing.assert_array_equal(got_offsets, offsets)
    out = inference.trace_paths(torch.from_numpy(parents.copy()).to(dev), torch.from_numpy(hops.copy()).to(dev),
                                torch.from_numpy(targets).to(dev), return_device_tensors=True)
    assert all(isinstance(o, torch.Tensor) and o.device.type == "cuda" for o in out)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int64
    np.testing.assert_array_equal(out[0].cpu().numpy(), paths)


def test_trace_every_foreground_voxel(dev):
    labels, sources, parents, hops = paths_case()
    targets = np.nonzero(hops.reshape(-1) >= 0)[0].astype(np.int32)
    check_paths(dev, labels.shape, parents, hops, targets)


def test_trace_counts_a_wrong_offsets_row_and_leaves_it_unwritten(dev):
    labels, sources, parents, hops = paths_case()
    reached = np.nonzero(hops.reshape(-1) >= 2)[0]
    targets = reached[[0, 5, 9, 14]].astype(np.int32)
    background = int(np.nonzero(hops.reshape(-1) < 0)[0][0])
    targets = np.concatenate([targets, np.array([background, -3, labels.size], dtype=np.int32)])
    lengths = np.where(np.arange(7) < 4, hops.reshape(-1)[np.clip(targets, 0, labels.size - 1)] + 1, 1).astype(np.int64)
    lengths[1] += 1      # a row that is one too long
    offsets = np.zeros(8, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    paths, _, state = run_trace(dev, parents, hops, targets, offsets=offsets)
    assert state == [4, 0]      # the long row, the background target and the two out of range
    for i in (0, 2, 3):
        np.testing.assert_array_equal(paths[offsets[i]:offsets[i + 1]], pref.walk(parents, hops, int(targets[i])))
    for i in (1, 4, 5, 6):
        assert (paths[offsets[i]:offsets[i + 1]] == -1).all()      # 0xFF bytes: unwritten
    # a row that would end beyond the capacity is refused on the device as well
    sound = np.zeros(5, dtype=np.int64)
    np.cumsum(hops.reshape(-1)[targets[:4]].astype(np.int64) + 1, out=sound[1:])
    paths, _, state = run_trace(dev, parents, hops, targets[:4], offsets=sound, capacity=int(sound[3]) + 1)
    assert state == [1, 0] and (paths[sound[3]:] == -1).all()


def test_trace_a_broken_chain_is_counted_and_nothing_is_read_out_of_range(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, parents, hops = paths_case()
    target = int(np.argmax(hops.reshape(-1)))
    path = pref.walk(parents, hops, target)
    assert len(path) >= 5
    for poison in (-1, labels.size, 2**31 - 1, path[2]):      # none, just outside, far outside, a self-parent
        broken = parents.copy()
        broken.reshape(-1)[path[2]] = poison      # one word mid-chain
        sound = int(next(v for v in np.nonzero(hops.reshape(-1) >= 1)[0] if path[2] not in pref.walk(parents, hops, v)))
        paths, offsets, state = run_trace(dev, broken, hops, np.array([target, sound], dtype=np.int32))
        assert state == [0, 1]      # guard words intact: run_trace checked them
        np.testing.assert_array_equal(paths[offsets[1]:offsets[2]], pref.walk(parents, hops, sound))
        with pytest.raises(RuntimeError, match="1 broken walk"):
            inference.trace_paths(broken, hops.copy(), np.array([target], dtype=np.int32))
    # a chain that ends on a voxel which is not its own parent
    broken = parents.copy()
    broken.reshape(-1)[path[0]] = path[1]
    assert run_trace(dev, broken, hops, np.array([target], dtype=np.int32))[2] == [0, 1]


# ---- 11. the chain -----------------------------------------------------------------------------------------
def test_from_agglomerate_affinities_to_the_paths_on_the_device(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    rng = np.random.default_rng(7)
    shape = (40, 48, 64)
    z, y, x = np.indices(shape)
    ball = ((z - 20) ** 2 + (y - 26) ** 2 + (x - 44) ** 2) <= 81      # a soma of radius 9
    inside = (((y - 10) ** 2 + (x - 14) ** 2) <= 25) | ball           # and a neurite along z
    for v in [(20, 26, 44), (20, 26, 45), (21, 26, 44)]:              # background voxels at the soma's centre
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
    dbf = inference.distance_to_boundary(filled, return_device_tensor=True)
    first = inference.segment_table(filled, n_labels=2, return_device_tensors=True)[3]
    _, _, roots = inference.geodesic_field(filled, first, return_farthest=True, return_device_tensors=True)
    daf, _, far_index = inference.geodesic_field(filled, roots, return_farthest=True, return_device_tensors=True)
    # TEASAR's penalty with three element-wise operations: dear near the boundary, a little dearer far from the root
    depth = dbf.to(torch.float32).sqrt()
    cost = torch.where(filled > 0, (1 - depth / depth.max()) ** 16 * 5000 + daf / daf.max() + 1e-3, 1.0)
    cost = cost.to(torch.float32).contiguous()
    pdrf = inference.geodesic_field(filled, roots, cost=cost, return_device_tensors=True)
    parents, hops = inference.geodesic_parents(filled, roots, field=pdrf, cost=cost, return_hops=True,
                                               return_device_tensors=True)
    voxels, offsets = inference.trace_paths(parents, hops, far_index[1:].contiguous(), return_device_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.device == labels.device for t in (parents, hops, voxels, offsets))

    want_labels, _ = holes_ref.by_components(host)
    np.testing.assert_array_equal(filled.cpu().numpy(), want_labels)
    want_first = ref.first_voxels(want_labels, 2)
    _, want_roots = ref.farthest(want_labels, want_first, ref.relaxation(want_labels, want_first))
    np.testing.assert_array_equal(roots.cpu().numpy(), want_roots)
    want_daf = ref.relaxation(want_labels, want_roots)
    _, want_far = ref.farthest(want_labels, want_roots, want_daf)
    np.testing.assert_array_equal(far_index.cpu().numpy(), want_far)
    host_cost = cost.cpu().numpy()      # an input of what follows
    want_field = ref.relaxation(want_labels, want_roots, host_cost)
    np.testing.assert_array_equal(ref.bits(pdrf.cpu().numpy()), ref.bits(want_field))
    want_parents, want_hops, orphans, invalid = pref.jacobi(want_labels, want_roots, want_field, host_cost)
    assert (orphans, invalid) == (0, 0)
    np.testing.assert_array_equal(hops.cpu().numpy(), want_hops)
    np.testing.assert_array_equal(parents.cpu().numpy(), want_parents)
    want_voxels, want_offsets = pref.paths(want_parents, want_hops, want_far[1:])
    np.testing.assert_array_equal(offsets.cpu().numpy(), want_offsets)
    np.testing.assert_array_equal(voxels.cpu().numpy(), want_voxels)
    neurite = int(host[0, 10, 14])
    row = want_voxels[want_offsets[neurite - 1]:want_offsets[neurite]]
    assert len(row) >= 40 and row[0] == want_roots[neurite] and row[-1] == want_far[neurite]      # end to end
