"""
exaspim_teasar_begin / _round / _apply and inference.teasar_branches / skeletonize_labels on the GPU (-m gpu).
Every comparison is array_equal on integers against the incremental oracle of tests/teasar_ref.py
(tests/test_teasar_ref_cpu.py holds it to the form that stamps whole cubes along whole paths): the state byte
of every voxel is downloaded and compared after EVERY round, then the vertices, radii, previous vertices,
offsets and the three per-branch arrays. Every run through the C ABI writes into buffers pre-filled with 0xFF
bytes between guard words that must not change. Nothing here provokes a fault: every refused call is rejected
on the host before a launch, and the walk of a spoiled parents array is bounded and range-checked.
"""

import numpy as np
import pytest
import torch

import geodesic_ref as ref
import holes_ref
import parents_ref as pref
import teasar_ref as tref
from aind_exaspim_neuron_segmentation_amd import _native

pytestmark = pytest.mark.gpu

GUARD = 64             # elements around every output
NAMES = ("labels", "sources", "dbf", "daf", "parents", "hops")


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


def run_teasar(dev, labels, sources, dbf, daf, parents, hops, scale, const, boxes=None, max_paths=None, limit=4096,
               keep_states=True):
    """
    begin, then round / one read / cumulative sum / apply until no label is live: through the C ABI into
    guarded, poisoned buffers. Returns a teasar_ref.Result with the state after every round.
    """
    lib = _native.lib()
    host = [np.array(a, dtype=t) for a, t in zip((labels, sources, dbf, daf, parents, hops),
                                                              (np.int32, np.int32, np.int32, np.float32, np.int32,
                                                               np.int32))]
    labels = host[0]
    shape, k, n = labels.shape, len(host[1]) - 1, labels.size
    if boxes is None:
        boxes = tref.boxes_of(labels, k)
    boxes = np.ascontiguousarray(boxes, dtype=np.int32)
    dims = _native.int3(shape)
    lab, src, dbf_d, daf_d, par, hop = (torch.from_numpy(a).to(dev) for a in host)
    box = torch.from_numpy(boxes).to(dev)
    need = lib.exaspim_teasar_workspace_bytes(dims, k)
    assert need >= 32, _native.last_error()
    mask_full, mask = guarded(dev, n, torch.uint8)
    state_full, state = guarded(dev, 5, torch.int32)
    ws_full, ws = guarded(dev, need, torch.uint8)      # GUARD = 64 bytes keeps the 16-byte alignment
    tgt_full, tgt = guarded(dev, k + 1, torch.int32)
    len_full, lengths = guarded(dev, k + 1, torch.int64)
    jun_full, junction = guarded(dev, k + 1, torch.int32)
    off_full, offsets = guarded(dev, k + 2, torch.int64)
    rc = lib.exaspim_teasar_begin(lab.data_ptr(), src.data_ptr(), hop.data_ptr(), daf_d.data_ptr(), dims, k,
                                  mask.data_ptr(), state.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, _native.last_error()
    out = tref.Result()
    out.initial = mask.cpu().numpy().reshape(shape)
    assert state.cpu().tolist() == [0] * 5
    out.refused = 0
    rounds = 0
    while max_paths is None or rounds < max_paths:
        assert rounds < limit, "no end"
        rc = lib.exaspim_teasar_round(lab.data_ptr(), daf_d.data_ptr(), par.data_ptr(), hop.data_ptr(), dims, k,
                                      mask.data_ptr(), tgt.data_ptr(), lengths.data_ptr(), junction.data_ptr(),
                                      state.data_ptr(), ws.data_ptr(), need, None)
        assert rc == 0, _native.last_error()
        live, broken, n_new, n_roots, refused = state.cpu().tolist()
        out.broken += broken
        if live == 0 and broken == 0:
            break
        rounds += 1
        host_lengths, host_junction, host_targets = lengths.cpu().numpy(), junction.cpu().numpy(), tgt.cpu().numpy()
        assert host_lengths[0] == 0 and host_junction[0] == -1 and host_targets[0] == -1
        assert int(host_lengths.sum()) == n_new and int((host_lengths > 0).sum()) == live
        assert int(((host_lengths > 0) & (host_junction < 0)).sum()) == n_roots
        offsets[0] = 0
        torch.cumsum(lengths, 0, out=offsets[1:])
        vox_full, vox = guarded(dev, n_new, torch.int32)
        rad_full, rad = guarded(dev, n_new, torch.int32)
        bef_full, bef = guarded(dev, n_new, torch.int32)
        rc = lib.exaspim_teasar_apply(lab.data_ptr(), par.data_ptr(), dbf_d.data_ptr(), box.data_ptr(), dims, k,
                                      float(scale), float(const), mask.data_ptr(), tgt.data_ptr(), lengths.data_ptr(),
                                      junction.data_ptr(), offsets.data_ptr(), vox.data_ptr() if n_new else None,
                                      rad.data_ptr() if n_new else None, bef.data_ptr() if n_new else None, n_new,
                                      n_new, n_roots, state.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0, _native.last_error()
        for full, count, dtype in ((vox_full, n_new, torch.int32), (rad_full, n_new, torch.int32),
                                   (bef_full, n_new, torch.int32)):
            assert intact(full, count, dtype)
        out.voxels += vox.cpu().tolist()
        out.radii += rad.cpu().tolist()
        out.before += bef.cpu().tolist()
        for row in np.nonzero(host_lengths)[0]:
            out.offsets.append(out.offsets[-1] + int(host_lengths[row]))
            out.branch_label.append(int(row))
            out.branch_round.append(rounds)
            out.branch_junction.append(int(host_junction[row]))
        out.live.append(live)
        out.new.append(n_new)
        if keep_states:
            out.states.append(mask.cpu().numpy().reshape(shape))
    out.refused = int(state.cpu()[4])
    out.final = mask.cpu().numpy().reshape(shape)
    assert intact(mask_full, n, torch.uint8) and intact(state_full, 5, torch.int32) and intact(ws_full, need, torch.uint8)
    assert intact(tgt_full, k + 1, torch.int32) and intact(len_full, k + 1, torch.int64)
    assert intact(jun_full, k + 1, torch.int32) and intact(off_full, k + 2, torch.int64)
    for got, want in zip((lab, src, dbf_d, par, hop, box), host[:3] + host[4:] + [boxes]):      # only read
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert daf_d.cpu().numpy().tobytes() == host[3].tobytes()
    return out


def same(got, want):
    """A device run against an oracle run: the state after every round, then every list."""
    assert got.broken == want.broken and got.refused == 0
    np.testing.assert_array_equal(got.initial, want.initial)
    assert len(got.states) == len(want.states), (len(got.states), len(want.states))
    for t, (a, b) in enumerate(zip(got.states, want.states)):
        np.testing.assert_array_equal(a, b, err_msg=f"the state after round {t + 1}")
    for name, a, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"),
                          got.arrays(), want.arrays()):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert got.before == want.before and got.live == want.live and got.new == want.new


def check(dev, inputs, scale, const, **kw):
    want = tref.incremental(*inputs, scale, const, **kw)
    got = run_teasar(dev, *inputs, scale, const, **kw)
    same(got, want)
    return got


# ---- 1. straight shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 31, 32, 33, 65, 200])
def test_lines_along_x(dev, w):
    for at in sorted({0, w // 2}):
        inputs = tref.line(w, 2, at)
        for scale, const in ((0.0, 0.0), (1.25, 0.0), (0.0, 3.0)):
            got = check(dev, inputs, scale, const)
            assert got.branch_junction[0] == -1 and got.voxels[0] == inputs[1][1]
            assert len(got.voxels) == w and not (got.final & tref.VALID).any()      # every voxel is on a path
            assert len(got.states) == (1 if at == 0 or w == 1 else 2)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("length", [7, 8, 9, 17])
def test_lines_along_z_and_y(dev, axis, length):
    for at in sorted({0, length // 2, length - 1}):
        got = check(dev, tref.line(length, axis, at), 1.25, 1.0)
        assert len(got.voxels) == length


# ---- 2. branching shapes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,const", [(0.0, 0.0), (0.0, 1.0), (1.25, 0.0)])
def test_a_y_and_a_comb_stop_at_their_junctions(dev, scale, const):
    inputs = tref.y_shape()
    got = check(dev, inputs, scale, const)
    fork = tref.index_of(inputs[0].shape, (1, 8, 10))
    assert got.branch_junction == [-1, fork] and got.new == [18, 5]
    inputs = tref.comb()
    got = check(dev, inputs, scale, const)
    # a tooth's lowest voxel (1, 2, 4 t) has the diagonal parent (1, 1, 4 t - 1): that is where its branch joins
    spine = [tref.index_of(inputs[0].shape, (1, 1, 4 * t - 1)) for t in (4, 3, 2, 1)]
    assert got.branch_junction[0] == -1 and got.new[0] == 26      # the spine up to x = 19 and the last tooth
    assert [j for j in got.branch_junction[1:] if j in spine] == spine      # the other teeth, farthest first
    assert all(got.new[got.branch_junction.index(j)] == 6 for j in spine)


def test_a_cross_breaks_its_ties_by_the_index(dev):
    inputs = tref.cross()
    shape = inputs[0].shape
    daf = inputs[3]
    assert len({daf[1, 0, 5].tobytes(), daf[1, 10, 5].tobytes(), daf[1, 5, 0].tobytes(), daf[1, 5, 10].tobytes()}) == 1
    got = check(dev, inputs, 0.0, 0.0)
    centre = tref.index_of(shape, (1, 5, 5))
    assert got.branch_junction == [-1, centre, centre, centre] and got.new == [6, 5, 5, 5]
    tips = [got.voxels[got.offsets[b + 1] - 1] for b in range(4)]
    assert tips == [tref.index_of(shape, v) for v in ((1, 0, 5), (1, 5, 0), (1, 5, 10), (1, 10, 5))]
    check(dev, inputs, 1.25, 1.0)


# ---- 3. neighbouring labels and the two clips ----------------------------------------------------------------
def touching_labels():
    shape = (6, 10, 40)
    labels = np.ones(shape, dtype=np.int32)
    labels[:, 5:, :] = 2      # the plane y = 4 | 5
    labels[0, 0, :3] = 0
    return labels


def test_touching_labels_keep_their_own_bytes(dev):
    labels = touching_labels()
    shape = labels.shape
    both = tref.case(labels, [-1, tref.index_of(shape, (3, 4, 0)), tref.index_of(shape, (3, 5, 39))])
    for scale, const in ((0.0, 2.0), (1.25, 3.0), (1.25, 450.0)):
        check(dev, both, scale, const)
    # with K = 1 the second label is no label of the loop: cubes of label 1 reach across, its bytes stay 0
    alone = tref.case(labels, [-1, tref.index_of(shape, (3, 4, 0))])
    got = check(dev, alone, 0.0, 3.0)
    assert all((s[labels == 2] == 0).all() for s in got.states) and len(got.states) > 1
    # label 2 rooted but cut after one round: label 1's cubes have reached into its half, its bytes are its own
    got = check(dev, both, 0.0, 6.0, max_paths=1)
    want_two = tref.incremental(*tref.case(np.where(labels == 2, 2, 0), [-1, -1, both[1][2]]), 0.0, 6.0, max_paths=1)
    np.testing.assert_array_equal(got.states[0][labels == 2], want_two.states[0][labels == 2])


def test_a_box_smaller_than_the_cube_and_a_label_on_every_face(dev):
    shape = (6, 7, 37)
    full = tref.case(np.ones(shape, dtype=np.int32), [-1, tref.index_of(shape, (2, 3, 5))])
    for scale, const in ((1.25, 450.0), (0.0, 2.0), (0.0, 0.0)):
        got = check(dev, full, scale, const, max_paths=3 if const == 0 else None)
        if const == 450.0:
            assert len(got.states) == 1 and set(got.radii) == {37} and not (got.final & tref.VALID).any()
    labels = np.zeros((9, 12, 44), dtype=np.int32)
    labels[2:5, 3:6, 4:40] = 1      # a bar whose cubes of radius 4 and 44 leave its box on every side
    labels[5:8, 3:9, 10:20] = 2     # a neighbour inside those cubes
    bar = tref.case(labels, [-1, tref.index_of(labels.shape, (3, 4, 4)), tref.index_of(labels.shape, (6, 4, 10))])
    for scale, const in ((0.0, 4.0), (1.25, 450.0), (0.0, 1.0)):
        check(dev, bar, scale, const)
    # boxes of the caller's that are tighter than the labels, reach out of the volume, or are empty
    boxes = np.array([[0] * 6, [2, 3, 4, 5, 6, 21], [-4, -4, -4, 99, 99, 99]], dtype=np.int32)
    got = check(dev, bar, 0.0, 4.0, boxes=boxes, max_paths=6)      # outside its box a label loses its vertices alone
    assert (got.final[2:5, 3:6, 30:40] & tref.VALID).any() and not (got.final[2:5, 3:6, 4:21] & tref.VALID).any()
    boxes[1] = [3, 3, 3, 3, 9, 9]
    check(dev, bar, 0.0, 4.0, boxes=boxes, max_paths=3)


# ---- 4. radii ------------------------------------------------------------------------------------------------
_WAVY = []


def wavy():
    if not _WAVY:
        inputs = tref.wavy_block()
        for a in inputs:
            a.setflags(write=False)
        _WAVY.append(inputs)
    return _WAVY[0]


@pytest.mark.parametrize("const", [0.0, 2.0])
def test_radii_that_rise_and_fall_along_a_path(dev, const):
    inputs = wavy()
    got = check(dev, inputs, 1.25, const)
    steps = set(np.diff(got.radii).tolist())
    assert min(steps) <= -2 and max(steps) >= 2 and 0 in steps      # growing, shrinking and equal neighbours
    census = tref.slab_census(got, inputs[0], inputs[2], 1.25, const)
    assert census == {"z-", "z+", "y-", "y+", "x-", "x+", "whole", "none"}, census


def test_one_voxel_per_vertex_needs_many_rounds(dev):
    shape = (3, 3, 12)
    inputs = tref.case(np.ones(shape, dtype=np.int32), [-1, 0])
    got = check(dev, inputs, 0.0, 0.0)
    assert set(got.radii) == {0} and len(got.voxels) == 108 and len(got.states) >= 20
    assert sorted(got.voxels) == list(range(108))      # every voxel ends on the skeleton


def line_65536(dbf_values):
    """A (1, 1, 65536) line with host-made parents and hops: x - 1 leads back to the source at 0."""
    n = 65536
    assert len(dbf_values) == n
    x = np.arange(n, dtype=np.int32)
    labels = np.ones((1, 1, n), dtype=np.int32)
    parents = np.maximum(x - 1, 0).reshape(1, 1, n)
    return (labels, np.array([-1, 0], dtype=np.int32), np.asarray(dbf_values, dtype=np.int32).reshape(1, 1, n),
            x.astype(np.float32).reshape(1, 1, n), parents, x.reshape(1, 1, n).copy())


def radius_values():
    """All of 0..4095, every k^2 and k^2 +- 1 up to 2^31 - 2, and DBF_INF: sorted, without repeats."""
    k = np.arange(0, 46341, dtype=np.int64)
    squares = np.concatenate([k * k - 1, k * k, k * k + 1])
    values = np.concatenate([np.arange(4096), squares[(squares >= 0) & (squares <= 2**31 - 2)], [tref.DBF_INF]])
    return np.unique(values).astype(np.int32)


@pytest.mark.parametrize("scale,const", [(1.25, 450.0), (1.0 / 3.0, 0.1), (1e-3, 0.0)])
def test_the_radius_arithmetic_is_numpys(dev, scale, const):
    values = radius_values()
    assert values[-1] == tref.DBF_INF and values[-2] == 46340 ** 2 + 1 <= 2**31 - 2 and len(values) > 2 * 65536
    for at in range(0, len(values), 65536):
        chunk = values[at:at + 65536]
        chunk = np.concatenate([chunk, np.full(65536 - len(chunk), -7, dtype=np.int32)])      # negative: as 0
        got = run_teasar(dev, *line_65536(chunk), scale, const, keep_states=False)
        want = tref.radius(chunk, scale, const, 65536)
        assert got.voxels == list(range(65536)) and got.before == [-1] + list(range(65535))
        np.testing.assert_array_equal(np.array(got.radii, dtype=np.int64), want)
        assert (got.final == tref.SKELETON).all() and got.broken == 0 and got.refused == 0 and got.new == [65536]
    assert int(np.sqrt(np.float64(2**31 - 2)) * 1.25 + 450.0) == 58376      # below the cap: the sum is what is floored


# ---- 5. degenerate labels and volumes ------------------------------------------------------------------------
def test_degenerate_labels(dev):
    shape = (5, 9, 40)
    labels = np.zeros(shape, dtype=np.int32)
    labels[2, 4, 7] = 1                    # a single voxel: its target is its root
    labels[1:3, 1:3, 20:30] = 2            # a label without a source
    labels[3:5, 6:9, 0:12] = 3             # one id in two pieces: the piece without the source is never valid
    labels[3:5, 6:9, 30:40] = 3
    labels[0, 0, 0:5] = 7                  # above K
    labels[0, 8, 0:5] = -2                 # negative
    sources = [-1, tref.index_of(shape, (2, 4, 7)), -1, tref.index_of(shape, (3, 6, 0)), -1]      # K = 4, 4 absent
    inputs = tref.case(labels, sources)
    got = check(dev, inputs, 0.0, 1.0)
    np.testing.assert_array_equal(got.initial != 0, (labels == 1) | ((labels == 3) & (np.indices(shape)[2] < 12)))
    first = got.branch_label.index(1)
    assert got.voxels[got.offsets[first]:got.offsets[first + 1]] == [sources[1]] and got.branch_round[first] == 1
    assert set(got.branch_label) == {1, 3}
    # a source row that names a voxel of another label makes the whole label ineligible
    wrong = list(sources)
    wrong[3] = sources[1]
    daf, parents, hops = inputs[3:]
    got = run_teasar(dev, labels, wrong, inputs[2], daf, parents, hops, 0.0, 1.0)
    same(got, tref.incremental(labels, np.array(wrong, dtype=np.int32), inputs[2], daf, parents, hops, 0.0, 1.0))
    assert set(got.branch_label) == {1}
    # daf words that are not finite and non-negative: -0.0, NaN, inf and negatives are never valid
    odd = daf.copy()
    odd[3, 6, 1], odd[3, 6, 2], odd[3, 6, 3], odd[3, 6, 4] = -0.0, np.nan, np.inf, -1.0
    got = run_teasar(dev, labels, sources, inputs[2], odd, parents, hops, 0.0, 0.0)
    same(got, tref.incremental(labels, inputs[1], inputs[2], odd, parents, hops, 0.0, 0.0))
    assert (got.initial[3, 6, 1:5] == 0).all() and got.initial[3, 6, 5] == 1


def test_degenerate_volumes(dev):
    nothing = np.zeros((4, 5, 33), dtype=np.int32)
    got = check(dev, tref.case(nothing, [-1, -1]), 1.25, 2.0)
    assert got.states == [] and got.voxels == [] and not got.final.any()
    got = check(dev, tref.case(nothing, [-1]), 1.25, 2.0)      # K = 0
    assert got.states == []
    one = tref.case(np.ones((1, 1, 1), dtype=np.int32), [-1, 0])
    for scale, const in ((0.0, 0.0), (1.25, 450.0)):
        got = check(dev, one, scale, const)
        assert got.voxels == [0] and got.final.tolist() == [[[tref.SKELETON]]] and got.branch_junction == [-1]
    got = check(dev, tref.case(np.zeros((1, 1, 1), dtype=np.int32), [-1, -1]), 0.0, 0.0)
    assert got.states == []


@pytest.mark.parametrize("max_paths", [1, 2])
def test_max_paths(dev, max_paths):
    from aind_exaspim_neuron_segmentation_amd import inference

    inputs = tref.comb()
    got = check(dev, inputs, 0.0, 1.0, max_paths=max_paths)
    assert len(got.states) == max_paths and (got.final & tref.VALID).any()
    stats = {}
    out = inference.teasar_branches(*(a.copy() for a in inputs), scale=0.0, const=1.0, max_paths=max_paths, stats=stats)
    for a, b in zip(out, got.arrays()):
        np.testing.assert_array_equal(a, b)
    assert stats["rounds"] == max_paths and stats["reads"] == max_paths + 1      # one per round and the last rows'
    assert stats["vertices"] == got.new and stats["live_labels"] == got.live


# ---- 6. more voxels than one launch covers -------------------------------------------------------------------
def test_launch_cap(dev):
    """
    (262152, 9, 9) has 21 234 312 voxels: the passes over the voxels launch 65536 workgroups of 256 threads
    and stride. Three blobs: at z = 0, straddling z = 262144 and at the far end, behind voxel 65536 * 256;
    each is compared on its own crop, the rest of the volume is background and must stay 0.
    """
    shape = (262152, 9, 9)
    assert int(np.prod(shape)) > 65536 * 256 and 262138 * 81 > 65536 * 256
    rng = np.random.default_rng(41)
    labels = np.zeros(shape, dtype=np.int32)
    spans = {1: (0, 6), 2: (262138, 262147), 3: (262148, 262152)}
    sources = np.full(4, -1, dtype=np.int32)
    for label, (z0, z1) in spans.items():
        block = rng.random((z1 - z0, 9, 9)) < 0.2
        block[:, 4, 4] = True      # a spine from the source through every plane of the blob
        labels[z0:z1][block] = label
        sources[label] = tref.index_of(shape, (z0, 4, 4))
    dbf = np.zeros(shape, dtype=np.int32)
    daf = np.zeros(shape, dtype=np.float32)
    parents = np.full(shape, -1, dtype=np.int32)
    hops = np.full(shape, -1, dtype=np.int32)
    crops = ((0, 8, (1,)), (262130, 262152, (2, 3)))
    wants = []
    for a, b, rows in crops:      # crops that hold whole labels
        local = np.full(4, -1, dtype=np.int32)
        for row in rows:
            local[row] = sources[row] - a * 81
        inputs = tref.case(labels[a:b], local)
        dbf[a:b], daf[a:b], hops[a:b] = inputs[2], inputs[3], inputs[5]
        parents[a:b] = np.where(inputs[4] >= 0, inputs[4] + a * 81, -1)
        wants.append(tref.incremental(*inputs, 0.0, 1.0))
    got = run_teasar(dev, labels, sources, dbf, daf, parents, hops, 0.0, 1.0)
    assert got.broken == 0 and got.refused == 0 and len(got.states) == max(len(w.states) for w in wants) >= 2
    outside = np.ones(shape[0], dtype=bool)
    for (a, b, rows), want in zip(crops, wants):
        outside[a:b] = False
        for t, state in enumerate(got.states):
            np.testing.assert_array_equal(state[a:b], want.states[min(t, len(want.states) - 1)], err_msg=f"round {t + 1}")
        for row in rows:
            mine = [(got.branch_round[i], got.branch_junction[i], got.voxels[got.offsets[i]:got.offsets[i + 1]])
                    for i in range(len(got.branch_label)) if got.branch_label[i] == row]
            theirs = [(want.branch_round[i], want.branch_junction[i] + a * 81 if want.branch_junction[i] >= 0 else -1,
                       [v + a * 81 for v in want.voxels[want.offsets[i]:want.offsets[i + 1]]])
                      for i in range(len(want.branch_label)) if want.branch_label[i] == row]
            assert mine == theirs and mine
    assert all(not state[outside].any() for state in (got.states[0], got.final))


# ---- 7. seeded volumes, determinism ----------------------------------------------------------------------------
SCALES = [(0.0, 0.0), (1.25, 0.0), (1.25, 2.0), (0.5, 1.0), (0.0, 3.0), (1.25, 450.0)]


@pytest.mark.parametrize("seed", range(30))
def test_seeded_volumes(dev, seed):
    """
    Every round's state against the oracle. The seeds that draw scale = const = 0 make one vertex per voxel and
    are cut at max_paths=40 for the run time: there the device is not held to the oracle down to an empty mask;
    test_one_voxel_per_vertex_needs_many_rounds runs 0 / 0 to the end.
    """
    shape = (24, 24, 40) if seed % 10 == 0 else None
    inputs = tref.seeded(seed, max_shape=(12, 12, 40), max_labels=5, shape=shape)
    scale, const = SCALES[seed % len(SCALES)]
    check(dev, inputs, scale, const, max_paths=40 if (scale, const) == (0.0, 0.0) else None)


def test_runs_repeat(dev):
    inputs = tref.seeded(10, shape=(24, 24, 40), max_labels=5)
    first = run_teasar(dev, *inputs, 1.25, 1.0)
    again = run_teasar(dev, *inputs, 1.25, 1.0)
    assert len(first.states) == len(again.states) >= 2
    for a, b in zip(first.states, again.states):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(first.arrays(), again.arrays()):
        assert a.tobytes() == b.tobytes()
    assert first.before == again.before


# ---- 8. spoiled parents ----------------------------------------------------------------------------------------
def test_a_broken_walk_is_counted_and_nothing_is_read_out_of_range(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels, sources, dbf, daf, parents, hops = tref.seeded(9)
    start = tref.eligible(labels, sources, hops, daf)
    target = int(np.argmax(np.where(start, daf, -1).reshape(-1)))
    chain = pref.walk(parents, hops, target)[::-1]      # target first
    assert len(chain) >= 5
    row = int(labels.reshape(-1)[target])
    for poison in (-1, labels.size, 2**31 - 1, chain[2]):      # none, just outside, far outside, an early self-parent
        spoiled = parents.copy()
        spoiled.reshape(-1)[chain[2]] = poison      # one word mid-chain
        got = run_teasar(dev, labels, sources, dbf, daf, spoiled, hops, 1.25, 0.0)      # the guards: run_teasar
        want = tref.incremental(labels, sources, dbf, daf, spoiled, hops, 1.25, 0.0)
        same(got, want)
        assert got.broken == 1 and row not in got.branch_label
        np.testing.assert_array_equal(got.final[labels == row], got.initial[labels == row])      # nothing written
        with pytest.raises(RuntimeError, match="1 broken walk"):
            inference.teasar_branches(labels.copy(), sources.copy(), dbf.copy(), daf.copy(), spoiled, hops.copy(),
                                      scale=1.25, const=0.0)
    # a chain that ends on a voxel which is not its own parent
    spoiled = parents.copy()
    spoiled.reshape(-1)[chain[-1]] = chain[-2]
    got = run_teasar(dev, labels, sources, dbf, daf, spoiled, hops, 1.25, 0.0)
    assert got.broken == 1 and row not in got.branch_label


# ---- 9. refusals -----------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched(dev):
    lib = _native.lib()
    shape, k = (5, 6, 36), 2
    n = int(np.prod(shape))
    host = np.ones(shape, dtype=np.int32)
    host[:, 3:] = 2
    inputs = tref.case(host, [-1, 0, n - 1])
    labels, sources, dbf, daf, parents, hops = (torch.from_numpy(a.copy()).to(dev) for a in inputs)
    boxes = torch.from_numpy(tref.boxes_of(host, k)).to(dev)
    need = lib.exaspim_teasar_workspace_bytes(_native.int3(shape), k)
    mask = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=dev)
    state = torch.full((5,), -7654321, dtype=torch.int32, device=dev)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device=dev)
    targets = torch.full((k + 1,), -1234567, dtype=torch.int32, device=dev)
    lengths = torch.full((k + 1,), -2345678, dtype=torch.int64, device=dev)
    junction = torch.full((k + 1,), -3456789, dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 0, 4, 8], dtype=torch.int64, device=dev)
    voxels = torch.full((128,), -4567890, dtype=torch.int32, device=dev)
    radii = torch.full((128,), -5678901, dtype=torch.int32, device=dev)
    before = torch.full((128,), -6789012, dtype=torch.int32, device=dev)
    values = dict(labels=labels.data_ptr(), sources=sources.data_ptr(), dbf=dbf.data_ptr(), daf=daf.data_ptr(),
                  parents=parents.data_ptr(), hops=hops.data_ptr(), boxes=boxes.data_ptr(), dims=_native.int3(shape),
                  k=k, scale=1.25, const=2.0, mask=mask.data_ptr(), state=state.data_ptr(), ws=ws.data_ptr(),
                  need=need, targets=targets.data_ptr(), lengths=lengths.data_ptr(), junction=junction.data_ptr(),
                  offsets=offsets.data_ptr(), voxels=voxels.data_ptr(), radii=radii.data_ptr(),
                  before=before.data_ptr(), n_new=8, capacity=128, n_roots=2, stream=None)
    calls = {
        "begin": (lib.exaspim_teasar_begin, ("labels", "sources", "hops", "daf", "dims", "k", "mask", "state", "ws",
                                             "need", "stream")),
        "round": (lib.exaspim_teasar_round, ("labels", "daf", "parents", "hops", "dims", "k", "mask", "targets",
                                             "lengths", "junction", "state", "ws", "need", "stream")),
        "apply": (lib.exaspim_teasar_apply, ("labels", "parents", "dbf", "boxes", "dims", "k", "scale", "const", "mask",
                                             "targets", "lengths", "junction", "offsets", "voxels", "radii", "before",
                                             "n_new", "capacity", "n_roots", "state", "stream")),
    }

    def call(which, **changes):
        fn, names = calls[which]
        rc = fn(*[changes.get(name, values[name]) for name in names])
        torch.cuda.synchronize()
        return rc

    def refused(which, code, what, **changes):
        assert set(changes) <= set(calls[which][1]), (which, changes)
        assert call(which, **changes) == code, (which, changes, _native.last_error())
        assert what in _native.last_error(), (which, changes, _native.last_error())
        assert (mask == 0x5A).all() and (state == -7654321).all() and (ws == 0xFF).all(), (which, changes)
        assert (targets == -1234567).all() and (lengths == -2345678).all() and (junction == -3456789).all()
        assert (voxels == -4567890).all() and (radii == -5678901).all() and (before == -6789012).all()
        np.testing.assert_array_equal(labels.cpu().numpy(), host)

    pointers = {"begin": ("labels", "sources", "hops", "daf", "mask", "state", "ws"),
                "round": ("labels", "daf", "parents", "hops", "mask", "targets", "lengths", "junction", "state", "ws"),
                "apply": ("labels", "parents", "dbf", "boxes", "mask", "targets", "lengths", "junction", "offsets",
                          "voxels", "radii", "before", "state")}
    for which, names in pointers.items():
        for name in names:
            refused(which, -1, "NULL", **{name: None})
            if name not in ("mask", "ws"):
                wide = name in ("lengths", "offsets")
                refused(which, -1, "misaligned", **{name: values[name] + (4 if wide else 2)})
        refused(which, -1, "dims", dims=_native.int3((5, 0, 36)))
        refused(which, -1, "dims", dims=_native.int3((5, -9, 36)))
        refused(which, -1, "dims", dims=_native.int3((2048, 1024, 1024)))      # 2^31 voxels
        refused(which, -1, "n_labels", k=-1)
        if which != "apply":
            refused(which, -1, "misaligned", ws=values["ws"] + 8)
            refused(which, -3, "workspace", need=need - 1)
            refused(which, -3, "workspace", need=0)
    for name in ("scale", "const"):
        for bad in (-1.0, -1e-300, float("inf"), -float("inf"), float("nan")):
            refused("apply", -1, "finite", **{name: bad})
    refused("apply", -1, "capacity", capacity=7)      # smaller than the offsets' total
    refused("apply", -1, "capacity", capacity=-1)
    refused("apply", -1, "n_new", n_new=-1)
    refused("apply", -1, "n_new", n_new=n + 1, capacity=n + 1)
    refused("apply", -1, "n_roots", n_roots=-1)
    assert lib.exaspim_teasar_workspace_bytes(_native.int3((5, 0, 36)), k) == 0 and "dims" in _native.last_error()
    assert lib.exaspim_teasar_workspace_bytes(_native.int3(shape), -1) == 0 and "n_labels" in _native.last_error()

    # the same buffers serve a sound run
    want = tref.incremental(*inputs, 1.25, 2.0)
    assert call("begin") == 0, _native.last_error()
    np.testing.assert_array_equal(mask[:n].cpu().numpy().reshape(shape), want.initial)
    assert (mask[n:] == 0x5A).all() and state.tolist() == [0] * 5
    assert call("round") == 0, _native.last_error()
    assert state.tolist() == [2, 0, want.new[0], 2, 0] and want.new[0] <= 128
    offsets = torch.zeros(k + 2, dtype=torch.int64, device=dev)
    torch.cumsum(lengths, 0, out=offsets[1:])
    assert call("apply", offsets=offsets.data_ptr(), n_new=want.new[0]) == 0, _native.last_error()
    np.testing.assert_array_equal(mask[:n].cpu().numpy().reshape(shape), want.states[0])
    assert voxels[:want.new[0]].tolist() == want.voxels[:want.new[0]] and (voxels[want.new[0]:] == -4567890).all()
    assert radii[:want.new[0]].tolist() == want.radii[:want.new[0]] and state.tolist()[4] == 0
    # offsets that do not belong to the lengths: the rows are counted and left unwritten, the state byte stays
    assert call("begin") == 0 and call("round") == 0
    voxels.fill_(-4567890)
    shifted = offsets + 1
    assert call("apply", offsets=shifted.data_ptr(), n_new=want.new[0]) == 0, _native.last_error()
    assert state.tolist()[4] >= 1 and (mask[n:] == 0x5A).all()


def test_python_layer_refusals(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    inputs = tref.case(np.ones((5, 6, 36), dtype=np.int32), [-1, 0])
    t = [torch.from_numpy(a.copy()).to(dev) for a in inputs]
    kw = dict(scale=1.25, const=2.0)
    with pytest.raises(TypeError, match="labels must be int32"):
        inference.teasar_branches(t[0].long(), *t[1:], **kw)
    with pytest.raises(TypeError, match="daf must be float32"):
        inference.teasar_branches(t[0], t[1], t[2], t[2], t[4], t[5], **kw)
    with pytest.raises(ValueError, match="hops must have the labels' shape"):
        inference.teasar_branches(*t[:5], t[5][:, :, :35], **kw)
    for i, name in enumerate(tref_names()):
        if i:
            moved = list(t)
            moved[i] = t[i].cpu()
            with pytest.raises(RuntimeError, match=f"{name} must be on the labels' device"):
                inference.teasar_branches(*moved, **kw)
    with pytest.raises(RuntimeError, match="boxes must be on the labels' device"):
        inference.teasar_branches(*t, boxes=torch.zeros((2, 6), dtype=torch.int32), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        inference.teasar_branches(*(a.cpu() for a in t), **kw)
    out = inference.teasar_branches(*t, return_device_tensors=True, n_labels=1, **kw)
    assert all(isinstance(o, torch.Tensor) and o.device == t[0].device for o in out)
    assert [o.dtype for o in out] == [torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32]
    for a, b in zip(out, tref.incremental(*inputs, 1.25, 2.0).arrays()):
        np.testing.assert_array_equal(a.cpu().numpy(), b)


def tref_names():
    return NAMES


# ---- 10. the Python layer and the chain --------------------------------------------------------------------------
def test_teasar_branches_equals_the_c_abi_and_counts_its_reads(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    inputs = tref.seeded(20, shape=(24, 24, 40), max_labels=5)
    want = tref.incremental(*inputs, 1.25, 1.0)
    stats = {}
    out = inference.teasar_branches(*(a.copy() for a in inputs), scale=1.25, const=1.0, stats=stats)
    assert [o.dtype for o in out] == [np.int32, np.int32, np.int64, np.int32, np.int32, np.int32]
    for a, b in zip(out, want.arrays()):
        np.testing.assert_array_equal(a, b)
    print(f"teasar_branches: {stats}")
    assert stats["rounds"] == len(want.states) >= 2 and stats["reads"] == stats["rounds"] + 1
    assert stats["vertices"] == want.new and stats["live_labels"] == want.live
    # boxes of the caller's
    again = inference.teasar_branches(*(a.copy() for a in inputs), scale=1.25, const=1.0,
                                      boxes=tref.boxes_of(inputs[0], len(inputs[1]) - 1))
    for a, b in zip(again, out):
        np.testing.assert_array_equal(a, b)


def test_skeletonize_labels_against_the_oracles(dev):
    from aind_exaspim_neuron_segmentation_amd import inference

    labels = np.ascontiguousarray(holes_ref.seeded_volume(7), dtype=np.int32)
    big = np.zeros((16, 20, 40), dtype=np.int32)
    big[1:1 + labels.shape[0], 2:2 + labels.shape[1], 3:3 + labels.shape[2]] = labels
    big[10:15, 14:19, 20:38] = 5      # a thick bar with an enclosed cavity
    big[12, 16, 25:28] = 0
    kw = dict(scale=1.25, const=2.0, pdrf_exponent=4, pdrf_scale=100000.0)
    chain = inference._skeleton_chain_on_device(torch.from_numpy(big).to(dev), kw["scale"], kw["const"], 4, 100000.0,
                                                True, None)
    filled, _ = holes_ref.by_components(big)
    assert filled[12, 16, 26] == 5
    np.testing.assert_array_equal(chain["labels"].cpu().numpy(), filled)
    k = int(filled.max())
    dbf = tref.dbf_of(filled)
    np.testing.assert_array_equal(chain["dbf"].cpu().numpy(), dbf)
    first = ref.first_voxels(filled, k)
    _, roots = ref.farthest(filled, first, ref.relaxation(filled, first))
    np.testing.assert_array_equal(chain["roots"].cpu().numpy(), roots)
    daf = ref.relaxation(filled, roots)
    np.testing.assert_array_equal(ref.bits(chain["daf"].cpu().numpy()), ref.bits(daf))
    cost = chain["cost"].cpu().numpy()      # an input of what follows; tests/test_gpu_penalty.py holds it to its oracle
    assert cost.dtype == np.float32 and np.isfinite(cost[np.isfinite(daf) & (filled > 0)]).all()
    field = ref.relaxation(filled, roots, cost)
    parents, hops, orphans, invalid = pref.jacobi(filled, roots, field, cost)
    assert (orphans, invalid) == (0, 0)
    np.testing.assert_array_equal(chain["parents"].cpu().numpy(), parents)
    want = tref.incremental(filled, roots, dbf, daf, parents, hops, kw["scale"], kw["const"])
    for name, b in zip(("voxels", "radii", "offsets", "branch_label", "branch_round", "branch_junction"), want.arrays()):
        np.testing.assert_array_equal(chain[name].cpu().numpy(), b, err_msg=name)
    assert chain["before"].cpu().tolist() == want.before and len(want.states) >= 2

    skeletons = inference.skeletonize_labels(big, **kw)
    sets = want.vertex_sets(k)
    assert sorted(skeletons) == [row for row in range(1, k + 1) if sets[row]] and len(skeletons) >= 2
    flat_parents, flat_labels, flat_dbf = parents.reshape(-1), filled.reshape(-1), dbf.reshape(-1)
    for row, (vertices, parent, radius) in skeletons.items():
        assert vertices.dtype == np.int32 and parent.dtype == np.int32 and radius.dtype == np.float32
        assert vertices.shape == (len(sets[row]), 3) and parent.shape == radius.shape == (len(sets[row]),)
        index = np.ravel_multi_index(tuple(vertices.T), big.shape)
        assert set(index.tolist()) == sets[row] and (flat_labels[index] == row).all()
        np.testing.assert_array_equal(radius, np.sqrt(flat_dbf[index].astype(np.float32)))
        root = np.nonzero(parent < 0)[0]
        assert root.tolist() == [0] and index[0] == roots[row]      # the root comes first
        rest = np.nonzero(parent >= 0)[0]
        assert (parent[rest] < len(index)).all() and (flat_labels[index[parent[rest]]] == row).all()
        np.testing.assert_array_equal(index[parent[rest]], flat_parents[index[rest]])      # taken from parents
        text = inference.skeleton_to_swc(vertices, parent, radius)
        assert len(text.splitlines()) == len(index) and text.splitlines()[0].endswith(" -1")
    unfilled = inference.skeletonize_labels(big, fill_holes=False, max_paths=1, **kw)
    assert sorted(unfilled) == sorted(skeletons) and all(len(v[0]) <= len(skeletons[r][0]) for r, v in unfilled.items())
