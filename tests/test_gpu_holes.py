"""
exaspim_fill_holes and inference.fill_holes on the GPU (-m gpu), array_equal against the CPU oracle written
from the definition (tests/holes_ref.py; tests/test_holes_ref_cpu.py holds its two forms to each other): the
hand-built cases, the seeded volumes, cavities that cross tile faces, every width around the 16-byte mask
path with an aligned and a misaligned labels pointer, a volume whose background is one hot cavity, a fully
coated volume, a volume with more tiles and voxels than one capped launch covers, in-place use, determinism,
the counts, every refusal, and the chain agglomerate_affinities -> fill_holes -> distance_to_boundary ->
segment_table on the device. Every run through the C ABI writes into buffers pre-filled with 0xFF bytes
between guard words that must not change. Nothing here provokes a fault: every refused call is rejected on
the host before a launch.
"""

import numpy as np
import pytest
import torch

import dbf_ref
import holes_ref
from aind_exaspim_neuron_segmentation_amd import _native

pytestmark = pytest.mark.gpu

TILE = (8, 8, 32)      # (z, y, x) of the LDS pass
GUARD = 64             # elements around every output
CASES = holes_ref.hand_cases()


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


def run_holes(dev, labels, in_place=False, misaligned=False):
    """
    exaspim_fill_holes through the C ABI into guarded, poisoned buffers: (filled labels, holes, voxels).
    in_place passes the labels' own buffer as the output; misaligned puts the labels one element past a
    16-byte boundary, so that the mask kernel takes its scalar form whatever the width.
    """
    lib = _native.lib()
    labels = np.array(labels, dtype=np.int32)      # a writable copy: torch.from_numpy wants one
    shape = labels.shape
    n = int(np.prod(shape))
    in_full, t = guarded(dev, n + 1, torch.int32)
    t = t[1:] if misaligned else t[:n]
    assert (t.data_ptr() % 16 == 0) != misaligned
    t.copy_(torch.from_numpy(labels).reshape(-1))
    need = lib.exaspim_fill_holes_workspace_bytes(_native.int3(shape))
    assert need >= 13 * n, _native.last_error()
    out_full, out = guarded(dev, n, torch.int32)
    counts_full, counts = guarded(dev, 2, torch.int64)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    target = t if in_place else out
    rc = lib.exaspim_fill_holes(t.data_ptr(), _native.int3(shape), target.data_ptr(), counts.data_ptr(),
                                ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert rc == 0, _native.last_error()
    assert intact(out_full, n, torch.int32) and intact(counts_full, 2, torch.int64)
    assert intact(ws_full, need, torch.uint8)
    typed = in_full.view(torch.int32)
    assert bool((typed[:GUARD + (1 if misaligned else 0)].view(torch.uint8) == 0xFF).all())
    assert bool((typed[GUARD + n + (1 if misaligned else 0):].view(torch.uint8) == 0xFF).all())
    if in_place:
        assert bool((out.view(torch.uint8) == 0xFF).all())      # the other buffer was not written
    else:
        np.testing.assert_array_equal(t.cpu().numpy().reshape(shape), labels)      # the input is only read
    holes, voxels = (int(v) for v in counts.cpu())
    return target.cpu().numpy().reshape(shape), holes, voxels


def check(dev, labels, want=None, **kw):
    """The C ABI against by_components (and against "want", an expectation by construction), counts included."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    oracle, stats = holes_ref.by_components(labels)
    if want is not None:
        np.testing.assert_array_equal(oracle, want)
    got, holes, voxels = run_holes(dev, labels, **kw)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, oracle)
    assert (holes, voxels) == (stats["filled"], stats["voxels"])
    return stats


# ---- 1. the hand-built cases ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,labels,want", CASES, ids=[c[0] for c in CASES])
def test_hand_built_case(dev, name, labels, want):
    from aind_exaspim_neuron_segmentation_amd import inference

    check(dev, labels, want)
    check(dev, labels, want, in_place=True)
    before, given = labels.copy(), labels.copy()
    got = inference.fill_holes(given)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got is not given
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(given, before)
    t = torch.from_numpy(labels.copy()).to(dev)
    on_device, holes, voxels = inference.fill_holes(t, return_counts=True, return_device_tensor=True)
    assert isinstance(on_device, torch.Tensor) and on_device.device == t.device and on_device.dtype == torch.int32
    assert on_device.data_ptr() != t.data_ptr()
    np.testing.assert_array_equal(on_device.cpu().numpy(), want)
    np.testing.assert_array_equal(t.cpu().numpy(), before)      # the argument is never mutated
    assert type(holes) is int and type(voxels) is int and voxels == int((want != labels).sum())


# ---- 2. the seeded volumes ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(holes_ref.SEEDS))
def test_seeded_volume(dev, seed):
    check(dev, holes_ref.seeded_volume(seed))


# ---- 3. cavities that cross tile faces --------------------------------------------------------------------
def test_cavities_across_tile_faces(dev):
    solid = np.full((20, 20, 70), 6, dtype=np.int32)
    labels = solid.copy()
    labels[3, 3, 31:33] = 0           # x = 31 | 32
    labels[3, 7:9, 5] = 0             # y = 7 | 8
    labels[7:9, 12, 5] = -2           # z = 7 | 8
    labels[15:17, 15:17, 63:65] = 0   # and one across x = 63 | 64 and z = 15 | 16 at once
    stats = check(dev, labels, solid)
    assert stats["filled"] == 4 and stats["voxels"] == 2 + 2 + 2 + 8


SNAKE = [(2, 2, 2), (2, 2, 67), (2, 17, 67), (17, 17, 67), (17, 17, 2), (17, 4, 2), (9, 4, 2), (9, 4, 40),
         (9, 12, 40), (12, 12, 40)]


@pytest.mark.parametrize("closed", [True, False])
def test_a_snake_through_a_solid_block(dev, closed):
    solid = np.full((20, 20, 70), 3, dtype=np.int32)
    labels = holes_ref.carve(solid.copy(), SNAKE)
    z, y, x = np.nonzero(labels == 0)
    tiles = {(a // TILE[0], b // TILE[1], c // TILE[2]) for a, b, c in zip(z, y, x)}
    assert len(tiles) >= 12      # the snake crosses tile faces along every axis
    if closed:
        stats = check(dev, labels, solid)
        assert stats["filled"] == 1 and stats["voxels"] == int((labels == 0).sum())
    else:
        holes_ref.carve(labels, [SNAKE[-1], (19, 12, 40)])      # its last end reaches the face z = 19
        stats = check(dev, labels, labels)
        assert stats == dict(filled=0, voxels=0, open=1, mixed=0)


# ---- 4. widths around the 16-byte mask path ---------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 257])
def test_widths_with_both_mask_forms(dev, w):
    rng = np.random.default_rng(500 + w)
    labels = holes_ref.punched(rng, holes_ref.blocky(rng, (9, 10, w), top=2, block=5), 0.12)
    stats = check(dev, labels)                      # 16-byte loads iff w % 4 == 0
    assert check(dev, labels, misaligned=True) == stats      # the scalar form whatever the width
    if w >= 31:
        assert stats["filled"] >= 1 and stats["open"] >= 1


# ---- 5. the hot component ---------------------------------------------------------------------------------
_HOT = []


def hot_case():
    """(labels, oracle, stats): sparse tubes of a few labels on a background that is one cavity, computed once."""
    if not _HOT:
        labels = np.zeros((64, 256, 256), dtype=np.int32)
        rng = np.random.default_rng(71)
        for k in range(24):      # tubes along x, three voxels wide, four labels
            z, y = int(rng.integers(3, 60)), 6 + 10 * k
            labels[z - 1:z + 2, y - 1:y + 2, 10:246] = 1 + k % 4
        holes = []
        for k in range(0, 24, 3):      # a thickened segment with hand-placed holes inside it
            y = 6 + 10 * k
            z = int(np.nonzero(labels[:, y, 100])[0][1])
            labels[z - 3:z + 4, y - 3:y + 4, 90:140] = 1 + k % 4
            for x in (95, 127, 128):      # one-voxel holes; 127 | 128 make one of two voxels across x tiles
                labels[z, y, x] = 0
                holes.append((z, y, x))
            labels[z + 1, y - 1:y + 2, 110:113] = -4      # nine negative voxels
        # one cavity bounded by two labels: tubes 0 (label 1) and 1 (label 2) joined by a bridge with a gap inside
        za, zb = (int(np.nonzero(labels[:, y, 200])[0][1]) for y in (6, 16))
        labels[min(za, zb) - 1:max(za, zb) + 2, 5:18, 199:202] = 0
        labels[min(za, zb) - 1:max(za, zb) + 2, 5:12, 199:202] = 1
        labels[min(za, zb) - 1:max(za, zb) + 2, 12:18, 199:202] = 2
        labels[za, 11:13, 200] = 0      # (za, 11, 200) lies in label 1, (za, 12, 200) in label 2
        oracle, stats = holes_ref.by_components(labels)
        labels.setflags(write=False)
        oracle.setflags(write=False)
        _HOT.append((labels, oracle, stats, holes, (za, 11, 200)))
    return _HOT[0]


def test_a_background_that_is_one_hot_cavity(dev):
    labels, oracle, stats, holes, mixed = hot_case()
    assert (labels <= 0).mean() > 0.9
    assert stats["open"] == 1 and stats["mixed"] == 1 and stats["filled"] == 8 * 3      # 2 + 1 holes and the negatives
    for z, y, x in holes:
        assert oracle[z, y, x] > 0
    assert oracle[mixed] == 0 and labels[mixed] == 0
    got, n_holes, n_voxels = run_holes(dev, labels)
    np.testing.assert_array_equal(got, oracle)
    assert (n_holes, n_voxels) == (stats["filled"], stats["voxels"]) == (24, 8 * (1 + 2 + 9))


# ---- 6. a fully coated volume -----------------------------------------------------------------------------
@pytest.mark.parametrize("second_label", [False, True])
def test_a_fully_coated_volume(dev, second_label):
    shape = (24, 40, 72)
    labels = np.full(shape, 1, dtype=np.int32)
    labels[1:-1, 1:-1, 1:-1] = 0      # one giant cavity behind a coat of one voxel
    if second_label:
        labels[11, 20, 40] = 2        # an island: the cavity's neighbours are {1, 2}
        stats = check(dev, labels, labels)
        assert stats == dict(filled=0, voxels=0, open=0, mixed=1)
    else:
        stats = check(dev, labels, np.full(shape, 1, dtype=np.int32))
        assert stats == dict(filled=1, voxels=22 * 38 * 70, open=0, mixed=0)


# ---- 7. more voxels and more tiles than one launch covers -------------------------------------------------
def test_grid_stride_tails(dev):
    """
    The per-voxel kernels launch at most 65536 workgroups of 256 threads and tile_pass at most 65536 workgroups
    of one tile each; beyond that they stride. (262152, 9, 9), the shape of test_gpu_components.py's stride
    case, has 65 538 tiles and 21.2M voxels, more than 65536 * 256; a width of 9 is the mask kernel's scalar form. No
    test reaches the cap of the 16-byte mask form, which takes four voxels per thread and would need more than
    65536 * 256 * 4 = 2^26 voxels. A solid label with hand-placed cavities: the expectation is the solid volume
    for the closed ones and the input for those opened to a face, by construction (no oracle of 21M voxels).
    """
    shape = (262152, 9, 9)
    n = int(np.prod(shape))
    tiles_zyx = tuple(-(-s // t) for s, t in zip(shape, TILE))
    assert n > 65536 * 256 and int(np.prod(tiles_zyx)) == 65538 and shape[2] % 4 != 0
    labels = np.full(shape, 5, dtype=np.int32)
    closed = [[(100, 4, 4)], [(230000, 3, 3)], [(230000, 7, 5), (230000, 7, 6)],
              [(262143, 4, 4), (262144, 4, 4)],      # across the face of the last tile layer
              [(262146, 2, 2)], [(262150, 7, 7), (262150, 7, 6)], [(262147, 7, 4), (262147, 7, 5)]]
    opened = [[(262151, 4, 4), (262150, 4, 4)], [(240000, 0, 4), (240000, 1, 4)], [(262148, 4, 8), (262148, 4, 7)]]
    for cavity in closed + opened:
        assert len(cavity) == 1 or sum(abs(a - b) for a, b in zip(*cavity)) == 1      # 2 x 1 x 1
        for v in cavity:
            labels[v] = 0
    want = np.full(shape, 5, dtype=np.int32)
    for cavity in opened:
        for v in cavity:
            want[v] = 0

    def tile_of(v):
        return ((v[0] // TILE[0]) * tiles_zyx[1] + v[1] // TILE[1]) * tiles_zyx[2] + v[2] // TILE[2]

    def index_of(v):
        return (v[0] * shape[1] + v[1]) * shape[2] + v[2]

    flat = [v for cavity in closed for v in cavity]
    assert any(tile_of(v) >= 65536 for v in flat) and any(tile_of(v) < 65536 for v in flat)
    assert any(index_of(v) >= 65536 * 256 for v in flat) and any(index_of(v) < 65536 * 256 for v in flat)
    assert any(tile_of(v) >= 65536 for cavity in opened for v in cavity)
    assert tile_of(closed[3][0]) < 65536 <= tile_of(closed[3][1])
    got, holes, voxels = run_holes(dev, labels)
    np.testing.assert_array_equal(got, want)
    assert holes == len(closed) and voxels == len(flat)


# ---- 8. in place, determinism ---------------------------------------------------------------------------
def test_in_place_equals_out_of_place_and_runs_repeat(dev):
    rng = np.random.default_rng(83)
    labels = holes_ref.punched(rng, holes_ref.blocky(rng, (33, 40, 132), top=3, block=11), 0.1)
    stats = check(dev, labels)
    assert stats["filled"] >= 20 and stats["open"] >= 1 and stats["mixed"] >= 1
    first = run_holes(dev, labels)
    again = run_holes(dev, labels)
    in_place = run_holes(dev, labels, in_place=True)
    shifted = run_holes(dev, labels, in_place=True, misaligned=True)
    for other in (again, in_place, shifted):
        assert other[0].tobytes() == first[0].tobytes() and other[1:] == first[1:]


# ---- 9. refusals, before anything is launched -----------------------------------------------------------
def test_refusals_leave_every_output_alone(dev):
    lib = _native.lib()
    shape = (5, 6, 36)
    n = int(np.prod(shape))
    host = holes_ref.punched(np.random.default_rng(89), np.full(shape, 2, dtype=np.int32), 0.1)
    labels = torch.from_numpy(host).to(dev)
    need = lib.exaspim_fill_holes_workspace_bytes(_native.int3(shape))
    out = torch.full((n,), -1234567, dtype=torch.int32, device=dev)
    counts = torch.full((2,), -7654321, dtype=torch.int64, device=dev)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    names = ["labels", "dims", "out", "counts", "ws", "need", "stream"]

    def call(**changes):
        args = [labels.data_ptr(), _native.int3(shape), out.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, None]
        for name, value in changes.items():
            args[names.index(name)] = value
        rc = lib.exaspim_fill_holes(*args)
        torch.cuda.synchronize()
        return rc

    def refused(code, what, **changes):
        assert call(**changes) == code, (changes, _native.last_error())
        assert what in _native.last_error(), (changes, _native.last_error())
        assert (out == -1234567).all() and (counts == -7654321).all() and (ws == 0xFF).all(), changes
        np.testing.assert_array_equal(labels.cpu().numpy(), host)

    for name in ("labels", "out", "counts", "ws"):
        refused(-1, "NULL", **{name: None})
    refused(-1, "dims", dims=_native.int3((5, 0, 36)))
    refused(-1, "dims", dims=_native.int3((5, -6, 36)))
    refused(-1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
    refused(-1, "misaligned", labels=labels.data_ptr() + 2)
    refused(-1, "misaligned", out=out.data_ptr() + 1)
    refused(-1, "misaligned", counts=counts.data_ptr() + 4)
    refused(-1, "misaligned", ws=ws.data_ptr() + 8)
    refused(-3, "workspace", need=need - 1)
    refused(-3, "workspace", need=0)
    assert call() == 0, _native.last_error()                        # the same buffers serve a sound call
    want, stats = holes_ref.by_components(host)
    np.testing.assert_array_equal(out.cpu().numpy().reshape(shape), want)
    assert counts.tolist() == [stats["filled"], stats["voxels"]]


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    host = np.full((5, 6, 36), 2, dtype=np.int32)
    t = torch.from_numpy(host).to(dev)
    for bad in (host.astype(np.int64), t.long(), t.float()):
        with pytest.raises(TypeError, match="int32"):
            inference.fill_holes(bad)
    with pytest.raises(TypeError):
        inference.fill_holes(host.tolist())
    for bad in (host[0], t[0], t[None]):
        with pytest.raises(ValueError, match=r"\(D, H, W\)"):
            inference.fill_holes(bad)
    with pytest.raises(ValueError, match="empty"):
        inference.fill_holes(t[:, :0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.fill_holes(torch.from_numpy(host.copy()))
    strided = torch.from_numpy(np.array(holes_ref.hand_cases()[0][1])).to(dev).permute(2, 1, 0)
    np.testing.assert_array_equal(inference.fill_holes(strided), 7)      # a view that is not contiguous is copied


# ---- 10. the chain ----------------------------------------------------------------------------------------
def test_from_agglomerate_affinities_to_the_segment_table_on_the_device(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    rng = np.random.default_rng(7)
    shape = (40, 48, 64)
    z, y, x = np.indices(shape)
    ball = ((z - 20) ** 2 + (y - 26) ** 2 + (x - 44) ** 2) <= 81      # a soma of radius 9
    inside = (((y - 10) ** 2 + (x - 14) ** 2) <= 25) | ball
    carved = [(20, 26, 44), (20, 26, 45), (21, 26, 44)]             # background voxels at the soma's centre
    for v in carved:
        inside[v] = False
    aff = np.full((3,) + shape, 0.05, dtype=np.float32)
    # an edge is on iff both of its ends are inside: the segments are exactly the components of "inside"
    aff[0, :-1][inside[:-1] & inside[1:]] = 0.9
    aff[1, :, :-1][inside[:, :-1] & inside[:, 1:]] = 0.9
    aff[2, :, :, :-1][inside[:, :, :-1] & inside[:, :, 1:]] = 0.9
    aff += rng.random((3,) + shape, dtype=np.float32) * 0.05
    labels = inference.agglomerate_affinities(torch.from_numpy(aff).to(dev), min_segment_size=10,
                                              return_device_tensor=True)
    host = labels.cpu().numpy()
    np.testing.assert_array_equal(host > 0, inside)
    soma = int(host[20, 26, 40])
    assert host.max() == 2 and soma > 0 and all(host[v] == 0 for v in carved)

    filled, counts = inference._fill_holes_on_device(labels)         # nothing leaves the device in between
    field = inference.distance_to_boundary(filled, return_device_tensor=True)
    table = inference.segment_table(filled, field, return_device_tensors=True)
    assert all(isinstance(t, torch.Tensor) and t.device == labels.device for t in (filled, counts, field) + table)

    want_labels, stats = holes_ref.by_components(host)
    assert stats["filled"] == 1 and stats["voxels"] == 3 and all(want_labels[v] == soma for v in carved)
    np.testing.assert_array_equal(filled.cpu().numpy(), want_labels)
    assert counts.tolist() == [1, 3]
    np.testing.assert_array_equal(labels.cpu().numpy(), host)        # the labels themselves are as they were
    want_field = dbf_ref.per_label(want_labels, False)
    np.testing.assert_array_equal(field.cpu().numpy(), want_field)
    for a, b in zip(table, dbf_ref.segment_table(want_labels, want_field)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)

    # the step matters: on the unfilled labels the soma's peak is another one, bounded from the inside
    unfilled = inference.segment_table(labels, inference.distance_to_boundary(labels, return_device_tensor=True))
    peak, peak_unfilled = int(table[2][soma].cpu()), int(unfilled[2][soma])
    assert peak == 82 and peak_unfilled < peak, (peak, peak_unfilled)      # 82 = 9^2 + 1: the nearest voxel outside
    other = 3 - soma
    assert int(table[2][other].cpu()) == int(unfilled[2][other])
