"""
exaspim_dbf / exaspim_segment_table and inference.distance_to_boundary / segment_table on the GPU
(-m gpu), array_equal against the CPU oracle written from the definition (tests/dbf_ref.py;
tests/test_dbf_ref_cpu.py holds its brute force and its scipy form to each other): rows around the
chunk of the x scan with runs that cross every chunk boundary, thin volumes and deep windows for the
y and z passes, a tall volume with more rows and voxels than one capped launch covers, the degenerate volumes, brute-force parity on seeded volumes, the pipeline from
agglomerate_affinities' device tensor, the table with absent and out-of-range ids and tied peaks,
determinism, and every refusal. Every run through the C ABI writes into buffers pre-filled with 0xFF
bytes whose guard bytes must not change. Nothing here provokes a fault: every refused call is rejected
on the host before a launch.
"""

import numpy as np
import pytest
import torch

import dbf_ref
from aind_exaspim_neuron_segmentation_amd import _native
from dbf_ref import DBF_INF

pytestmark = pytest.mark.gpu

CHUNK = 256      # voxels of a row the x pass scans at once
GUARD = 64       # elements around every output
MODES = [False, True]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def guarded(dev, n, dtype):
    """A 0xFF-filled buffer of GUARD + n + GUARD elements."""
    full = torch.full(((n + 2 * GUARD) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8,
                      device=dev)
    return full, full.view(dtype)[GUARD:GUARD + n]


def intact(full, n, dtype):
    """The guard elements on both sides of a guarded() buffer still hold 0xFF bytes."""
    typed = full.view(dtype)
    return bool((typed[:GUARD].view(torch.uint8) == 0xFF).all() and (typed[GUARD + n:].view(torch.uint8) == 0xFF).all())


def run_dbf(dev, labels, border):
    """exaspim_dbf through the C ABI into a guarded, poisoned buffer."""
    lib = _native.lib()
    shape = labels.shape
    n = int(np.prod(shape))
    t = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    need = lib.exaspim_dbf_workspace_bytes(_native.int3(shape))
    assert need >= 4 * n, _native.last_error()
    full, out = guarded(dev, n, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    rc = lib.exaspim_dbf(t.data_ptr(), _native.int3(shape), int(border), out.data_ptr(), ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(full, n, torch.int32) and intact(ws_full, need, torch.uint8)
    np.testing.assert_array_equal(t.cpu().numpy(), labels)      # the input is only read
    return out.cpu().numpy().reshape(shape)


def check_dbf(dev, labels, oracle=dbf_ref.per_label, modes=MODES):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    for border in modes:
        want = oracle(labels, border)
        got = run_dbf(dev, labels, border)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg=f"black_border={border}")


# ---- 1. the x scan: chunks and carries ---------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_rows_around_the_chunk(dev, w):
    rng = np.random.default_rng(w)
    labels = dbf_ref.stretched_labels(rng, (3, 5, w), top=3, longest=max(2, min(w, 300)))
    if w == 600:
        assert any((labels[z, y, CHUNK - 1] == labels[z, y, CHUNK]) and labels[z, y, CHUNK] > 0
                   for z in range(3) for y in range(5))      # a run crosses a chunk boundary
    check_dbf(dev, labels)


def test_a_row_that_is_one_run(dev):
    labels = dbf_ref.stretched_labels(np.random.default_rng(1), (3, 5, 600), top=3, longest=150)
    labels[1, 2, :] = 2      # a single run of 600: both carries cross two chunk boundaries
    labels[1, 3, :] = 2
    labels[1, 3, 0] = 0      # and one bounded on the left only
    labels[1, 4, :] = 2
    labels[1, 4, 599] = 1    # on the right only
    check_dbf(dev, labels)
    alone = np.full((1, 1, 600), 5, dtype=np.int32)
    got = run_dbf(dev, alone, False)
    assert (got == DBF_INF).all()
    x = np.arange(600)
    assert (run_dbf(dev, alone, True) == 1).all()      # the border layer across the two unit axes
    alone[0, 0, 300] = 0
    np.testing.assert_array_equal(run_dbf(dev, alone, False).reshape(-1), (x - 300) ** 2)


# ---- 2. the y and z windows ---------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [1, 0])
@pytest.mark.parametrize("length", [1, 63, 65, 130])
def test_thin_volumes_along_y_and_z(dev, axis, length):
    rng = np.random.default_rng(100 * axis + length)
    long_first = dbf_ref.stretched_labels(rng, (2, 3, length), top=2, longest=max(2, length // 2))
    labels = np.ascontiguousarray(np.moveaxis(long_first, 2, axis))      # (2, length, 3) or (length, 2, 3)
    assert labels.shape[axis] == length
    check_dbf(dev, labels)


@pytest.fixture(scope="module")
def ball():
    z, y, x = np.indices((48, 48, 48))
    labels = (((z - 23) ** 2 + (y - 24) ** 2 + (x - 22) ** 2) <= 400).astype(np.int32) * 9
    return labels, {border: dbf_ref.per_label(labels, border) for border in MODES}


def test_a_ball_of_radius_20(dev, ball):
    labels, want = ball
    assert want[False].max() >= 400      # the windows go 20 deep
    for border in MODES:
        np.testing.assert_array_equal(run_dbf(dev, labels, border), want[border])


def test_two_halves_without_background(dev):
    for axis in range(3):
        labels = np.ones((20, 22, 70), dtype=np.int32)
        cut = labels.shape[axis] // 2
        index = [slice(None)] * 3
        index[axis] = slice(cut, None)
        labels[tuple(index)] = 2
        c = np.indices(labels.shape)[axis]
        want = np.where(c < cut, cut - c, c - cut + 1) ** 2      # the distance to the interface only
        np.testing.assert_array_equal(run_dbf(dev, labels, False), want)
        np.testing.assert_array_equal(run_dbf(dev, labels, True), dbf_ref.per_label(labels, True))


# ---- 2b. more rows and more voxels than one capped launch covers ----------------------------------------
def test_grid_stride_over_rows_and_voxels(dev):
    """
    dbf_x launches at most 65536 workgroups of one row each and dbf_axis at most 65536 of 256 voxels; beyond
    that they stride, dbf_x with its LDS table of chunk carries and its register carry rebuilt per row.
    (4, 21961, 260) has 87 844 rows and 22.8M voxels: 1830 blocks of (4, 11, 260) between zero rows, drawn
    from 64 with runs of up to 300 voxels (a row is two chunks) and one that is a single label, so the oracle
    is composed of 65 small ones (dbf_ref.tiled_rows; no EDT of the whole volume, and no axis beyond 46 339).
    """
    rng = np.random.default_rng(59)
    blocks = [dbf_ref.stretched_labels(rng, (4, 11, 260), top=3, longest=300) for _ in range(64)]
    blocks.append(np.full((4, 11, 260), 3, dtype=np.int32))
    assert all(((b[:, :, CHUNK - 1] == b[:, :, CHUNK]) & (b[:, :, CHUNK] > 0)).any() for b in blocks)   # across the chunk
    choice = rng.integers(0, len(blocks), size=1830)
    # plane z = 3 (rows 65883 on, voxels 17.1M on) lies wholly in the second trip of all three passes
    assert len(set(choice.tolist())) == len(blocks) and 3 * 21961 > 65536 and 3 * 21961 * 260 > 65536 * 256
    for border in MODES:
        labels, want = dbf_ref.tiled_rows(blocks, choice, border)
        d, h, w = labels.shape
        assert (d, h, w) == (4, 21961, 260)
        assert d * h > 65536 and d * h * w > 65536 * 256
        got = run_dbf(dev, labels, border)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg=f"black_border={border}")


# ---- 3. degenerate volumes ----------------------------------------------------------------------------
def test_degenerate_volumes(dev):
    for border in MODES:
        assert not run_dbf(dev, np.zeros((5, 6, 70), dtype=np.int32), border).any()
    solid = np.full((24, 24, 24), 4, dtype=np.int32)
    assert (run_dbf(dev, solid, False) == DBF_INF).all()
    c = np.indices(solid.shape)
    face = np.minimum(c + 1, 24 - c).min(axis=0)
    np.testing.assert_array_equal(run_dbf(dev, solid, True), face ** 2)
    checker = (np.indices((9, 10, 67)).sum(axis=0) % 2 + 1).astype(np.int32)
    for border in MODES:
        assert (run_dbf(dev, checker, border) == 1).all()
    extreme = np.full((6, 7, 66), 2**31 - 1, dtype=np.int32)
    extreme[2:4, 3:6, 10:40] = -(2**31)
    extreme[5, :, :] = -1
    extreme[0, 0, :] = 2**31 - 2
    check_dbf(dev, extreme)
    assert run_dbf(dev, np.ones((1, 1, 1), dtype=np.int32), False).item() == DBF_INF
    assert run_dbf(dev, np.ones((1, 1, 1), dtype=np.int32), True).item() == 1
    assert run_dbf(dev, np.zeros((1, 1, 1), dtype=np.int32), True).item() == 0


# ---- 4. brute-force parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(30))
def test_brute_force_parity(dev, seed):
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(1, 13, size=3))
    if seed % 3 == 0:
        labels = rng.integers(0, 4, size=shape)
    elif seed % 3 == 1:
        labels = rng.integers(-1, 3, size=shape) * rng.integers(0, 2, size=shape)
    else:
        labels = (rng.random(shape) < 0.9).astype(np.int64) * rng.integers(1, 3)      # mostly one label: deep windows
    check_dbf(dev, labels, oracle=dbf_ref.brute_force)


# ---- 5. the pipeline ----------------------------------------------------------------------------------
def test_from_agglomerate_affinities_on_the_device(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    rng = np.random.default_rng(7)
    shape = (40, 48, 64)
    # neurite-like: two thick tubes and a slab of high affinity in a low floor
    z, y, x = np.indices(shape)
    inside = (((y - 12) ** 2 + (x - 20) ** 2) <= 36) | (((z - 25) ** 2 + (y - 34) ** 2) <= 49) | (np.abs(x - 52) <= 3)
    aff = np.where(inside[None], 0.9, 0.05).astype(np.float32) + rng.random((3,) + shape, dtype=np.float32) * 0.05
    labels = inference.agglomerate_affinities(torch.from_numpy(aff).to(dev), min_segment_size=10,
                                              return_device_tensor=True)
    host = labels.cpu().numpy()
    assert host.max() >= 2 and (host == 0).any()
    for border in MODES:
        want = dbf_ref.per_label(host, border)
        got = inference.distance_to_boundary(labels, black_border=border, return_device_tensor=True)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int32 and got.device == labels.device
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        from_host = inference.distance_to_boundary(host, black_border=border)
        assert isinstance(from_host, np.ndarray) and from_host.dtype == np.int32
        np.testing.assert_array_equal(from_host, want)
    assert want.max() >= 16
    # and the table a skeletoniser would download with it
    table = inference.segment_table(labels, got)
    for a, b in zip(table, dbf_ref.segment_table(host, want)):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(inference.distance_to_boundary(labels), dbf_ref.per_label(host, False))


# ---- 6. the segment table -------------------------------------------------------------------------------
def run_table(dev, labels, dbf, k):
    """exaspim_segment_table through the C ABI into guarded, poisoned buffers."""
    lib = _native.lib()
    shape = labels.shape
    t = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    f = None if dbf is None else torch.from_numpy(np.ascontiguousarray(dbf)).to(dev)
    need = lib.exaspim_segment_table_workspace_bytes(k)
    assert need >= 8 * (k + 1), _native.last_error()
    kinds = [(k + 1, torch.int64), (6 * (k + 1), torch.int32), (k + 1, torch.int32), (k + 1, torch.int32),
             (need, torch.uint8)]
    bufs = [guarded(dev, n, dtype) for n, dtype in kinds]
    rc = lib.exaspim_segment_table(t.data_ptr(), None if f is None else f.data_ptr(), _native.int3(shape), k,
                                   *[view.data_ptr() for _, view in bufs], need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    for (full, _), (n, dtype) in zip(bufs, kinds):
        assert intact(full, n, dtype), dtype
    np.testing.assert_array_equal(t.cpu().numpy(), labels)
    sizes, boxes, peak, index = (view.cpu().numpy() for _, view in bufs[:4])
    return sizes, boxes.reshape(k + 1, 6), peak, index


def check_table(dev, labels, dbf, k):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    want = dbf_ref.segment_table(labels, dbf, k)
    got = run_table(dev, labels, dbf, k)
    for name, a, b in zip(("sizes", "boxes", "peak", "peak_index"), got, want):
        assert a.dtype == b.dtype, name
        np.testing.assert_array_equal(a, b, err_msg=name)
    return got


@pytest.mark.parametrize("with_dbf", [False, True])
def test_table_with_gaps_and_ids_out_of_range(dev, with_dbf):
    rng = np.random.default_rng(11)
    labels = dbf_ref.stretched_labels(rng, (9, 10, 67), top=12, longest=20)
    labels[labels == 5] = 0
    labels[labels == 9] = 3                                      # absent ids below the maximum
    labels[rng.random(labels.shape) < 0.05] = -7                 # negative
    labels[rng.random(labels.shape) < 0.05] = 2**31 - 1          # above any n_labels
    labels[rng.random(labels.shape) < 0.05] = -(2**31)
    dbf = rng.integers(0, 6, size=labels.shape).astype(np.int32) if with_dbf else None      # ties everywhere
    for k in (12, 20, 7, 1, 0):                                  # ids above n_labels are in the volume
        sizes, boxes, peak, index = check_table(dev, labels, dbf, k)
        assert sizes[0] == (labels == 0).sum()
    assert sizes.shape == (1,) and index[0] == -1


def test_table_of_a_solid_cube_takes_the_smallest_index(dev):
    labels = np.zeros((14, 15, 70), dtype=np.int32)
    labels[2:12, 3:13, 5:15] = 2                                  # 10^3: the peak 25 ties at 2^3 voxels
    dbf = run_dbf(dev, labels, True)
    sizes, boxes, peak, index = check_table(dev, labels, dbf, 2)
    assert sizes[2] == 1000 and list(boxes[2]) == [2, 3, 5, 12, 13, 15] and peak[2] == 25
    assert (dbf == 25).sum() == 8
    assert np.unravel_index(index[2], labels.shape) == (6, 7, 9)
    assert sizes[1] == 0 and index[1] == -1 and not boxes[1].any()
    whole = np.full((12, 12, 12), 1, dtype=np.int32)             # and the whole volume, in both modes
    check_table(dev, whole, run_dbf(dev, whole, True), 1)
    sizes, boxes, peak, index = check_table(dev, whole, run_dbf(dev, whole, False), 1)
    assert peak[1] == DBF_INF and index[1] == 0


def test_table_runs_that_straddle_wave_boundaries(dev):
    rng = np.random.default_rng(13)
    labels = dbf_ref.stretched_labels(rng, (3, 5, 257), top=3, longest=200)      # rows of 257: every wave is shifted
    labels[1, 1, :] = 3
    labels[1, 2, :] = 3                                           # one label across a row end: two runs
    dbf = rng.integers(0, 1000, size=labels.shape).astype(np.int32)
    check_table(dev, labels, dbf, 3)
    check_table(dev, labels, None, 3)
    check_table(dev, labels, -dbf, 3)                            # "the largest value" holds for any int32 field


def test_table_with_more_labels_than_a_workgroup_pools(dev):
    """2^22 voxels of noise in 0 .. 20 000: the pass strides 4 096 workgroups over the volume, each sees some 1 000
    labels, twice the slots of its LDS pool, so many run lengths take the way straight to the table."""
    rng = np.random.default_rng(37)
    shape, k = (64, 256, 256), 20000
    labels = rng.integers(0, k + 1, size=shape, dtype=np.int32)
    dbf = rng.integers(0, 50, size=shape, dtype=np.int32)
    want = dbf_ref.segment_table_sorted(labels, dbf, k)
    lib = _native.lib()
    t, f = torch.from_numpy(labels).to(dev), torch.from_numpy(dbf).to(dev)
    need = lib.exaspim_segment_table_workspace_bytes(k)
    outs = [torch.empty(k + 1, dtype=torch.int64, device=dev), torch.empty((k + 1, 6), dtype=torch.int32, device=dev),
            torch.empty(k + 1, dtype=torch.int32, device=dev), torch.empty(k + 1, dtype=torch.int32, device=dev)]
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.exaspim_segment_table(t.data_ptr(), f.data_ptr(), _native.int3(shape), k, *[o.data_ptr() for o in outs],
                                   ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    for name, a, b in zip(("sizes", "boxes", "peak", "peak_index"), outs, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=name)
    assert int(want[0].sum()) == labels.size


def test_public_segment_table(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    rng = np.random.default_rng(17)
    labels = dbf_ref.stretched_labels(rng, (7, 9, 40), top=6, longest=9)
    labels[labels == 6] = -2
    dbf = dbf_ref.per_label(labels, False)
    want = dbf_ref.segment_table(labels, dbf)
    got = inference.segment_table(labels, dbf)                   # numpy in, numpy out, n_labels from the volume
    for a, b in zip(got, want):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    assert got[0].shape == (6,)
    t = torch.from_numpy(labels).to(dev)
    on_device = inference.segment_table(t, n_labels=8, return_device_tensors=True)
    for a, b in zip(on_device, dbf_ref.segment_table(labels, None, 8)):
        assert isinstance(a, torch.Tensor) and a.device == t.device
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    assert on_device[1].shape == (9, 6)
    negative = inference.segment_table(np.full((2, 3, 4), -5, dtype=np.int32))      # max(labels.max(), 0)
    assert negative[0].tolist() == [0] and negative[3].tolist() == [-1]


# ---- 7. determinism -------------------------------------------------------------------------------------
def test_both_functions_are_deterministic(dev):
    rng = np.random.default_rng(19)
    labels = dbf_ref.stretched_labels(rng, (33, 40, 130), top=5, longest=60)
    first = run_dbf(dev, labels, True)
    np.testing.assert_array_equal(run_dbf(dev, labels, True), first)
    np.testing.assert_array_equal(first, dbf_ref.per_label(labels, True))
    a = run_table(dev, labels, first, 5)
    b = run_table(dev, labels, first, 5)
    assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
    for got, want in zip(a, dbf_ref.segment_table(labels, first, 5)):
        np.testing.assert_array_equal(got, want)


# ---- 8. refusals, before anything is launched -----------------------------------------------------------
def test_dbf_refusals(dev):
    lib = _native.lib()
    shape = (5, 6, 36)
    n = int(np.prod(shape))
    host = dbf_ref.stretched_labels(np.random.default_rng(23), shape)
    labels = torch.from_numpy(host).to(dev)
    need = lib.exaspim_dbf_workspace_bytes(_native.int3(shape))
    out = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    names = ["labels", "dims", "border", "out", "ws", "need", "stream"]

    def call(**changes):
        args = [labels.data_ptr(), _native.int3(shape), 0, out.data_ptr(), ws.data_ptr(), need, None]
        for name, value in changes.items():
            args[names.index(name)] = value
        rc = lib.exaspim_dbf(*args)
        torch.cuda.synchronize()
        return rc

    def refused(code, what, **changes):
        assert call(**changes) == code, (changes, _native.last_error())
        assert what in _native.last_error(), (changes, _native.last_error())
        assert (out == -1234567).all() and (ws == 0xFF).all(), changes      # nothing was launched

    for name in ("labels", "out", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "dims", dims=_native.int3((5, 0, 36)))
    refused(-1, "dims", dims=_native.int3((5, -6, 36)))
    refused(-1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
    refused(-1, "dims", dims=_native.int3((1, 1, 46341)))           # the squared diagonal
    refused(-1, "dims", dims=_native.int3((1, 1, 46340)))
    refused(-1, "misaligned", labels=labels.data_ptr() + 2)
    refused(-1, "misaligned", out=out.data_ptr() + 1)
    refused(-1, "misaligned", ws=ws.data_ptr() + 8)
    refused(-3, "workspace", need=need - 1)
    refused(-3, "workspace", need=0)
    assert call() == 0, _native.last_error()                        # the same buffers serve a sound call
    np.testing.assert_array_equal(out.cpu().numpy().reshape(shape), dbf_ref.per_label(host, False))


def test_segment_table_refusals(dev):
    lib = _native.lib()
    shape, k = (5, 6, 36), 3
    host = dbf_ref.stretched_labels(np.random.default_rng(29), shape)
    labels = torch.from_numpy(host).to(dev)
    dbf = torch.from_numpy(dbf_ref.per_label(host, False)).to(dev)
    need = lib.exaspim_segment_table_workspace_bytes(k)
    sizes = torch.full((k + 1,), -1234567, dtype=torch.int64, device=dev)
    boxes = torch.full((6 * (k + 1),), -1234567, dtype=torch.int32, device=dev)
    peak = torch.full((k + 1,), -1234567, dtype=torch.int32, device=dev)
    index = torch.full((k + 1,), -1234567, dtype=torch.int32, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    names = ["labels", "dbf", "dims", "k", "sizes", "boxes", "peak", "index", "ws", "need", "stream"]

    def call(**changes):
        args = [labels.data_ptr(), dbf.data_ptr(), _native.int3(shape), k, sizes.data_ptr(), boxes.data_ptr(),
                peak.data_ptr(), index.data_ptr(), ws.data_ptr(), need, None]
        for name, value in changes.items():
            args[names.index(name)] = value
        rc = lib.exaspim_segment_table(*args)
        torch.cuda.synchronize()
        return rc

    def refused(code, what, **changes):
        assert call(**changes) == code, (changes, _native.last_error())
        assert what in _native.last_error(), (changes, _native.last_error())
        for t in (sizes, boxes, peak, index):
            assert (t == -1234567).all(), changes
        assert (ws == 0xFF).all(), changes

    for name in ("labels", "sizes", "boxes", "peak", "index", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "dims", dims=_native.int3((5, 0, 36)))
    refused(-1, "dims", dims=_native.int3((2048, 1024, 1024)))
    refused(-1, "dims", dims=_native.int3((1, 1, 46341)))
    refused(-1, "n_labels", k=-1)
    refused(-1, "misaligned", labels=labels.data_ptr() + 2)
    refused(-1, "misaligned", dbf=dbf.data_ptr() + 2)
    refused(-1, "misaligned", sizes=sizes.data_ptr() + 4)
    refused(-1, "misaligned", boxes=boxes.data_ptr() + 2)
    refused(-1, "misaligned", peak=peak.data_ptr() + 1)
    refused(-1, "misaligned", index=index.data_ptr() + 2)
    refused(-1, "misaligned", ws=ws.data_ptr() + 8)
    refused(-3, "workspace", need=need - 1)
    refused(-3, "workspace", need=0)
    assert call(dbf=None) == 0, _native.last_error()                # dbf_dev alone may be NULL
    want = dbf_ref.segment_table(host, None, k)
    np.testing.assert_array_equal(sizes.cpu().numpy(), want[0])
    np.testing.assert_array_equal(index.cpu().numpy(), want[3])


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    host = dbf_ref.stretched_labels(np.random.default_rng(31), (5, 6, 36))
    t = torch.from_numpy(host).to(dev)
    for fn in (inference.distance_to_boundary, inference.segment_table):
        for bad in (host.astype(np.int64), t.long(), t.float()):
            with pytest.raises(TypeError, match="int32"):
                fn(bad)
        with pytest.raises(TypeError):
            fn(host.tolist())
        for bad in (host[0], t[0], t[None]):
            with pytest.raises(ValueError, match=r"\(D, H, W\)"):
                fn(bad)
        with pytest.raises(ValueError, match="empty"):
            fn(t[:, :0])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.from_numpy(host.copy()))
        with pytest.raises(ValueError, match="dims"):              # the library's refusal, through last_error
            fn(torch.zeros((1, 1, 46340), dtype=torch.int32, device=dev))
    with pytest.raises(TypeError, match="dbf must be int32"):
        inference.segment_table(t, t.long())
    with pytest.raises(ValueError, match="labels' shape"):
        inference.segment_table(t, t[:2])
    with pytest.raises(RuntimeError, match="labels' device"):
        inference.segment_table(t, torch.from_numpy(host.copy()))
    with pytest.raises(ValueError, match="n_labels"):
        inference.segment_table(t, n_labels=-1)
